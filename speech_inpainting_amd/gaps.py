"""Several gaps per clip: the host arithmetic of the multi-gap route (pure Python, no GPU).

A gap is a pair (first 20 ms frame, frame count) and means what the reference's single mask means (I_ea/predict.py:99-102,132-134,
164-168): 16 kHz samples [p * 320 + 80, (p + l) * 320 - 1) are zeroed, 22.05 kHz samples [p * 320 * 22050 // 16000,
(p + l) * 320 * 22050 // 16000) are zeroed, encoder frames [p, p + l) are decided and mel frames [p, p + l) replaced.  A clip carries
0 .. MAX_SPANS gaps, sorted and disjoint; the functions here validate them, turn them into the span tables (samples) and the frame
table (clip, frame) the library's `_spans` entry points take, and plan the generator windows of the diagnostics passes.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

MAX_SPANS = 16          # SI_MAX_SPANS of include/si_hip.h: spans per clip
MAX_CHANNELS = 8        # SI_MAX_CHANNELS of include/si_hip.h: channels of an interleaved file

Gap = Tuple[int, int]


def _is_pair(e) -> bool:
    try:
        p, l = e
        int(p), int(l)
        return True
    except (TypeError, ValueError):
        return False


def normalize_gaps(gaps: Sequence[Sequence[Sequence[int]]], limits: Optional[Sequence[int]] = None) -> List[List[Gap]]:
    """Per clip: the gaps sorted by first frame, as (pos, len) int pairs.  Raises a ValueError naming the clip and the gap for a
    frame count <= 0, a gap outside [0, limits[clip]) (the clip's min(T, Tm): the frames that exist on the encoder AND the mel
    side), overlapping gaps (touching ones are fine) and more than MAX_SPANS gaps in one clip."""
    out: List[List[Gap]] = []
    for b, clip in enumerate(gaps):
        try:
            g = sorted((int(p), int(l)) for p, l in clip)
        except (TypeError, ValueError):
            bad = next((k for k, e in enumerate(clip) if not _is_pair(e)), None)
            raise ValueError(f"clip {b}: gap {bad} = {clip[bad] if bad is not None else clip!r} is not a (first frame, frame count) pair") from None
        if len(g) > MAX_SPANS:
            raise ValueError(f"clip {b}: {len(g)} gaps, more than the {MAX_SPANS} a clip may carry")
        for k, (p, l) in enumerate(g):
            if l <= 0:
                raise ValueError(f"clip {b}: gap {k} = ({p}, {l}) has no frames")
            if p < 0 or (limits is not None and p + l > int(limits[b])):
                lim = "" if limits is None else f" ({int(limits[b])} frames on both sides)"
                raise ValueError(f"clip {b}: gap {k} = frames [{p}, {p + l}) does not fit the clip{lim}")
            if k and p < g[k - 1][0] + g[k - 1][1]:
                raise ValueError(f"clip {b}: gap {k} = frames [{p}, {p + l}) overlaps gap {k - 1} = "
                                 f"[{g[k - 1][0]}, {g[k - 1][0] + g[k - 1][1]})")
        out.append(g)
    return out


def spans16(gaps: Sequence[Sequence[Gap]]) -> List[List[Gap]]:
    """(start, len) in 16 kHz samples per gap: `mask_samples_from_frames` (I_ea/predict.py:133)."""
    return [[(p * 320 + 80, max((p + l) * 320 - 1 - (p * 320 + 80), 0)) for p, l in clip] for clip in gaps]


def spans22(gaps: Sequence[Sequence[Gap]], n22: Optional[Sequence[int]] = None) -> List[List[Gap]]:
    """(start, len) in 22.05 kHz samples per gap (I_ea/predict.py:99-100: the 16 kHz positions scaled by 22050 // 16000 after the
    product), clamped to the clip's n22[b] samples when given."""
    out = []
    for b, clip in enumerate(gaps):
        row = []
        for p, l in clip:
            s, e = p * 320 * 22050 // 16000, (p + l) * 320 * 22050 // 16000
            if n22 is not None:
                s, e = min(s, int(n22[b])), min(e, int(n22[b]))
            row.append((s, e - s))
        out.append(row)
    return out


def clamp_spans22(spans22: Sequence[Sequence[Sequence[int]]], n22: Sequence[int]) -> List[List[Gap]]:
    """Explicit 22.05 kHz spans, per clip [start, end) sample pairs (the `mask22` of predict_clips): sorted, clamped to the clip's
    n22[b] samples, as (start, len)."""
    out = []
    for clip, n in zip(spans22, n22):
        row = []
        for a, e in sorted((int(a), int(e)) for a, e in clip):
            a = min(max(a, 0), int(n))
            row.append((a, max(min(e, int(n)) - a, 0)))
        out.append(row)
    return out


def csr(spans: Sequence[Sequence[Gap]]) -> Tuple[List[int], List[int], List[int]]:
    """Per-clip (start, len) lists -> the CSR arrays (off (B + 1), start, len) of si_span_table."""
    off, st, ln = [0], [], []
    for clip in spans:
        for s, l in clip:
            st.append(int(s))
            ln.append(int(l))
        off.append(len(st))
    return off, st, ln


def frame_table(gaps: Sequence[Sequence[Gap]]) -> Tuple[List[int], List[int], List[int]]:
    """The masked frames of all gaps of all clips, flattened clip by clip, gap by gap: (clip index (F), frame (F), label_off (B + 1));
    clip b's labels are entries [label_off[b], label_off[b + 1]) of the flat label vector."""
    clip_idx, pos, off = [], [], [0]
    for b, clip in enumerate(gaps):
        for p, l in clip:
            clip_idx += [b] * l
            pos += list(range(p, p + l))
        off.append(len(pos))
    return clip_idx, pos, off


def stretched_range(p: int, l: int, t_out: int) -> Tuple[int, int]:
    """Frames of the x441/256 stretched mel whose two source frames touch mel frames [p, p + l) (one frame of slack each side)."""
    r = 441.0 / 256.0
    c0 = max(int(math.floor((p - 0.5) * r - 0.5)) - 1, 0)
    c1 = min(int(math.ceil((p + l + 0.5) * r - 0.5)) + 1, t_out)
    return c0, c1


def plan_windows(ranges: Sequence[Gap], t_out: int, rf: int) -> List[Tuple[int, int]]:
    """Generator windows [w0, w1) (stretched frames) for one clip whose mel changed in the frame ranges `ranges` = (pos, len) pairs.
    A window is the changed stretched frames widened by 2 * rf (rf = the generator's receptive radius in frames) and clamped to the
    clip; of its output the outer rf frames at an edge that is not a clip edge are dropped (they miss neighbours), the rest -- its
    KEPT region, which holds every frame within rf of a changed one -- is spliced back.  Windows that overlap or touch are merged
    (so are, a fortiori, windows whose kept regions do): the result is sorted and disjoint, and one range gives `vocode_window`'s
    single window."""
    wins: List[Tuple[int, int]] = []
    for p, l in sorted((int(p), int(l)) for p, l in ranges):
        c0, c1 = stretched_range(p, l, t_out)
        w0, w1 = max(c0 - 2 * rf, 0), min(c1 + 2 * rf, t_out)
        if wins and w0 <= wins[-1][1]:
            wins[-1] = (wins[-1][0], max(wins[-1][1], w1))
        else:
            wins.append((w0, w1))
    return wins


def kept_region(w0: int, w1: int, t_out: int, rf: int) -> Tuple[int, int]:
    """The frames of window [w0, w1) whose output is spliced back."""
    return w0 + (rf if w0 > 0 else 0), w1 - (rf if w1 < t_out else 0)


# ---- patch mode: the generated audio of the gaps spliced into the caller's own 22.05 kHz samples
def fade_ramp(fade: int):
    """The rising half of the cross-fade, fp32 (fade): w[i] = 0.5 * (1 - cos(pi * (i + 0.5) / fade)), computed in float64 and rounded
    once.  The compose kernel READS this table (it evaluates no cosine), so host and device weights are the same floats.
    fade = 0 gives an empty table: a hard splice."""
    import numpy as np
    fade = int(fade)
    if fade < 0:
        raise ValueError(f"fade = {fade} samples is negative")
    i = np.arange(fade, dtype=np.float64)
    return (0.5 * (1.0 - np.cos(np.pi * (i + 0.5) / max(fade, 1)))).astype(np.float32)


def blend_regions(spans22_b: Sequence[Gap], n22_b: int, n_out_b: int, fade: int) -> List[Optional[Gap]]:
    """Per (start, len) span of ONE clip (22.05 kHz samples) the half-open sample range [a, b) in which the patched output is not
    the original: the span widened by `fade` on each side, clamped to [0, lim), lim = min(n22_b, n_out_b) (the generator emits
    n_out_b <= n22_b samples; past them the original stays).  None for a span of length 0 and for one that starts at or past lim."""
    lim = min(int(n22_b), int(n_out_b))
    out: List[Optional[Gap]] = []
    for s, l in spans22_b:
        s, e = int(s), int(s) + int(l)
        out.append(None if l <= 0 or s >= lim else (max(s - fade, 0), min(e + fade, lim)))
    return out


def blend_weights(spans22_b: Sequence[Gap], n22_b: int, n_out_b: int, fade: int, n: Optional[int] = None):
    """The weight of the generated audio at every sample of one clip, fp32 (n or n22_b): per span ramp[m - (s - fade)] on the rise,
    1 inside [s, e), ramp[e + fade - 1 - m] on the fall; the MAXIMUM over the clip's spans (ramps overlap when two gaps are closer
    than 2 * fade); 0 elsewhere and for every m >= lim.  What patch_compose_kernel computes, as a host table for tests and tools."""
    import numpy as np
    ramp = fade_ramp(fade)
    w = np.zeros(int(n22_b) if n is None else int(n), dtype=np.float32)
    lim = min(int(n22_b), int(n_out_b), w.size)
    for (s, l), reg in zip(spans22_b, blend_regions(spans22_b, n22_b, n_out_b, fade)):
        if reg is None:
            continue
        s, e = int(s), int(s) + int(l)
        one = np.zeros_like(w)
        m = np.arange(reg[0], min(reg[1], lim))
        one[m] = np.where(m < s, ramp[np.clip(m - (s - fade), 0, max(fade - 1, 0))] if fade else 0.0,
                          np.where(m < e, 1.0, ramp[np.clip(e + fade - 1 - m, 0, max(fade - 1, 0))] if fade else 0.0))
        w = np.maximum(w, one)
    return w


def plan_patch_windows(regions: Sequence[Optional[Gap]], t_out: int, hop: int, rf: int) -> Tuple[List[Tuple[int, int]], List[int]]:
    """Generator windows [w0, w1) (stretched frames) for one clip's blend regions (`blend_regions`; None entries get no window).
    A region [a, b) needs stretched frames [a // hop, ceil(b / hop)); the window is that range widened by rf on each side and
    clamped to [0, t_out), so the needed frames lie in its kept region (`kept_region`).  Windows that overlap or touch are merged:
    only the needed samples must be exact here, not everything a changed frame can reach, hence rf and not `plan_windows`' 2 * rf.
    -> (windows sorted and disjoint, per region the index of its window or -1)."""
    order = sorted((k for k, r in enumerate(regions) if r is not None), key=lambda k: regions[k])
    wins: List[Tuple[int, int]] = []
    which = [-1] * len(regions)
    for k in order:
        a, b = regions[k]
        w0, w1 = max(a // hop - rf, 0), min(-(-b // hop) + rf, t_out)
        if wins and w0 <= wins[-1][1]:
            wins[-1] = (wins[-1][0], max(wins[-1][1], w1))
        else:
            wins.append((w0, w1))
        which[k] = len(wins) - 1
    for k in order:
        a, b = regions[k]
        k0, k1 = kept_region(*wins[which[k]], t_out, rf)
        assert k0 * hop <= a and b <= k1 * hop, f"region [{a}, {b}) leaves the kept frames [{k0}, {k1}) of its window"
    return wins, which


# ---- recordings longer than one clip: gaps on the recording's frame grid -> context clips
PC_CHUNK = 2048         # samples per workgroup of patch_regions_kernel (patch_kernels.hip)


def channel_gap_lists(gaps, channel_gaps, channels: int) -> List[list]:
    """One gap list per channel of an interleaved file: `gaps` for every channel, or channel_gaps as it is (a sequence
    of `channels` lists, any of them empty).  Both, neither, or a channel_gaps of another length raise a ValueError."""
    if gaps is not None and channel_gaps is not None:
        raise ValueError("both gaps and channel_gaps: one list for every channel, or one list per channel")
    if channel_gaps is None:
        if gaps is None:
            raise ValueError("neither gaps nor channel_gaps")
        return [list(gaps) for _ in range(int(channels))]
    per = [list(g) for g in channel_gaps]
    if len(per) != int(channels):
        raise ValueError(f"channel_gaps holds {len(per)} lists for a file of {int(channels)} channels")
    return per


def plan_channel_contexts(channel_gaps: Sequence[Sequence[Sequence[int]]], n_rec_frames: int, clip_frames: int = 200, min_context: int = 50,
                          lim_frames: Optional[int] = None, fade_frames: int = 1):
    """The contexts of an interleaved file: plan_contexts as it stands on each channel's own gap list -- a channel is
    a mono recording --, concatenated in (channel, start) order.  Each context carries "channel"; its own_index counts over ALL
    channels' sorted gaps in (channel, gap) order.  -> (contexts, channel_off): channel_off has one entry per channel + 1, the gaps
    of channel c are [channel_off[c], channel_off[c + 1]).  A ValueError of plan_contexts names the channel in front."""
    ctxs, off = [], [0]
    for c, g in enumerate(channel_gaps):
        try:
            own = plan_contexts(g, n_rec_frames, clip_frames, min_context, lim_frames=lim_frames, fade_frames=fade_frames)
        except ValueError as e:
            raise ValueError(f"channel {c}: {e}") from None
        for k in own:
            k["channel"] = c
            k["own_index"] = [off[-1] + i for i in k["own_index"]]
        ctxs += own
        off.append(off[-1] + len(g))
    return ctxs, off


def pass_channels(ctxs: Sequence[dict]) -> List[Tuple[int, int, int]]:
    """The contexts of ONE pass, in (channel, start) order, -> (channel, first row, end row) per channel present: its clips are
    consecutive rows of the pass, one cut and one write-back launch each."""
    out: List[Tuple[int, int, int]] = []
    for r, k in enumerate(ctxs):
        c = int(k["channel"])
        if out and out[-1][0] == c:
            out[-1] = (c, out[-1][1], r + 1)
        else:
            out.append((c, r, r + 1))
    return out


def gap_label_off(ctxs: Sequence[dict], n_gaps: int) -> List[int]:
    """label_off of a plan: gap k (own_index) of n_gaps owns labels [label_off[k], label_off[k + 1]), one per frame of the gap."""
    counts = [0] * int(n_gaps)
    for k in ctxs:
        for i, (_, l) in zip(k["own_index"], k["own"]):
            counts[i] = int(l)
    off = [0]
    for n in counts:
        off.append(off[-1] + n)
    return off


def plan_contexts(gaps: Sequence[Sequence[int]], n_rec_frames: int, clip_frames: int = 200, min_context: int = 50,
                  lim_frames: Optional[int] = None, fade_frames: int = 1) -> List[dict]:
    """Gaps of a RECORDING, (first frame, frame count) pairs on its 20 ms grid of n_rec_frames frames, -> the context clips that serve
    them.  The gaps are sorted and grouped greedily: a group starts with the first ungrouped gap and takes the next one while
    (that gap's end - the group's first start) <= clip_frames - 2 * min_context, up to MAX_SPANS gaps.  A group's context is
    min(clip_frames, n_rec_frames) frames long and starts at frame clamp((first start + last end) // 2 - clip_frames // 2, 0,
    max(n_rec_frames - clip_frames, 0)): every own gap has at least min_context frames of the recording on each side unless the
    recording ends there.  A recording of at most clip_frames frames is ONE context that owns every gap.
    lim_frames: the frames of a context clip that exist on the encoder AND the mel side (`gap_tables`' min(T, Tm)); default = all.
    -> per context a dict: start (frame), frames, own (the group's gaps, LOCAL frames), own_index (their places in the sorted gap
    list), foreign (every other gap that meets the context's usable frames [0, lim), clipped to them, local frames: its samples are
    unknown, so it is masked, predicted and spliced in the pass like an own gap, but never composed from this context).
    Raises a ValueError naming the gap in RECORDING frames for: a non-pair entry, a frame count <= 0, a gap outside [0, n_rec_frames),
    overlapping gaps, a gap longer than clip_frames - 2 * min_context, an own gap that does not fit [0, lim) of its context (a gap
    in the recording's last frame: the encoder has one frame fewer than the mel), own + foreign gaps above MAX_SPANS, and two gaps of
    DIFFERENT groups fewer than 2 * fade_frames frames apart (their cross-fades, fade_frames frames on each side, would overlap
    across contexts -- it takes a cluster of gaps longer than clip_frames - 2 * min_context)."""
    n_rec, clip, ctx_min, ff = int(n_rec_frames), int(clip_frames), int(min_context), int(fade_frames)
    if clip <= 0 or ctx_min < 0 or clip - 2 * ctx_min <= 0 or ff < 0:
        raise ValueError(f"plan_contexts: clip_frames = {clip}, min_context = {ctx_min}, fade_frames = {ff}: the clip must be longer than two contexts")
    try:
        g = sorted((int(p), int(l)) for p, l in gaps)
    except (TypeError, ValueError):
        bad = next((k for k, e in enumerate(gaps) if not _is_pair(e)), None)
        raise ValueError(f"recording: gap {bad} = {gaps[bad] if bad is not None else gaps!r} is not a (first frame, frame count) pair") from None
    budget = clip - 2 * ctx_min
    for k, (p, l) in enumerate(g):
        if l <= 0:
            raise ValueError(f"recording: gap {k} = ({p}, {l}) has no frames")
        if p < 0 or p + l > n_rec:
            raise ValueError(f"recording: gap {k} = frames [{p}, {p + l}) does not fit the recording ({n_rec} frames)")
        if k and p < g[k - 1][0] + g[k - 1][1]:
            raise ValueError(f"recording: gap {k} = frames [{p}, {p + l}) overlaps gap {k - 1} = [{g[k - 1][0]}, {g[k - 1][0] + g[k - 1][1]})")
    n_ctx = min(clip, n_rec)
    lim = n_ctx if lim_frames is None else min(int(lim_frames), n_ctx)
    groups: List[List[int]] = []
    if n_rec <= clip:
        if len(g) > MAX_SPANS:
            raise ValueError(f"recording: {len(g)} gaps in one context of {n_rec} frames, more than the {MAX_SPANS} a clip may carry")
        groups = [list(range(len(g)))] if g else []
    else:
        for k, (p, l) in enumerate(g):
            if l > budget:
                raise ValueError(f"recording: gap {k} = frames [{p}, {p + l}) is longer than the {budget} frames a context of {clip} frames "
                                 f"leaves between two contexts of {ctx_min}")
            if groups and len(groups[-1]) < MAX_SPANS and p + l - g[groups[-1][0]][0] <= budget:
                groups[-1].append(k)
            else:
                groups.append([k])
    group_of = {k: i for i, grp in enumerate(groups) for k in grp}
    for k in range(1, len(g)):
        if group_of[k] != group_of[k - 1] and g[k][0] - (g[k - 1][0] + g[k - 1][1]) < 2 * ff:
            raise ValueError(f"recording: gap {k} = frames [{g[k][0]}, {g[k][0] + g[k][1]}) lies {g[k][0] - g[k - 1][0] - g[k - 1][1]} frames after gap "
                             f"{k - 1}, which another context serves: their cross-fades ({ff} frames each side) would overlap across contexts")
    out = []
    for grp in groups:
        first, last = g[grp[0]][0], g[grp[-1]][0] + g[grp[-1]][1]
        f = min(max((first + last) // 2 - clip // 2, 0), max(n_rec - clip, 0))
        own, foreign = [], []
        for k, (p, l) in enumerate(g):
            if k in grp:
                if p - f < 0 or p + l - f > lim:
                    raise ValueError(f"recording: gap {k} = frames [{p}, {p + l}) does not fit the usable frames [{f}, {f + lim}) of its context")
                own.append((p - f, l))
            else:
                a, b = max(p, f), min(p + l, f + lim)
                if a < b:
                    foreign.append((a - f, b - a))
        if len(own) + len(foreign) > MAX_SPANS:
            k = grp[0]
            raise ValueError(f"recording: the context of gap {k} = frames [{g[k][0]}, {g[k][0] + g[k][1]}) holds {len(own)} gaps of its own and "
                             f"{len(foreign)} of other contexts, more than the {MAX_SPANS} a clip may carry")
        out.append({"start": f, "frames": n_ctx, "own": own, "own_index": list(grp), "foreign": foreign})
    return out


def region_chunks(regions: Sequence[Gap], chunk: int = PC_CHUNK) -> List[Tuple[int, int, int]]:
    """Blend regions [a, b) on the recording's sample axis, sorted by a with non-decreasing b (sorted disjoint spans widened by one
    fade), -> the chunks of `chunk` samples they touch, strictly increasing, each as (chunk index, k0, k1): regions [k0, k1) are
    the ones that meet it.  The chunk list of si_region_table: one workgroup per entry."""
    out: List[Tuple[int, int, int]] = []
    for k, (a, b) in enumerate(regions):
        a, b = int(a), int(b)
        if b <= a:
            raise ValueError(f"region {k} = [{a}, {b}) is empty")
        if k and (a < int(regions[k - 1][0]) or b < int(regions[k - 1][1])):
            raise ValueError(f"region {k} = [{a}, {b}) is not sorted after region {k - 1}")
        for c in range(a // chunk, (b - 1) // chunk + 1):
            j = len(out) - 1
            while j >= 0 and out[j][0] > c:
                j -= 1
            if j >= 0 and out[j][0] == c:
                out[j] = (c, out[j][1], k + 1)
            else:
                out.append((c, k, k + 1))
    return out


# ---- dropout detection: runs of quiet samples at any file rate -> gaps on the recording's 20 ms grid
def runs_to_gaps(runs: Sequence[Sequence[int]], n: int, sr: int, n_rec_frames: int, lim_frames: Optional[int] = None, pad_frames: int = 0,
                 merge_frames: int = 2, max_frames: int = 20) -> Tuple[List[Gap], List[Tuple[int, int, str]]]:
    """Runs of quiet samples, (start, len) pairs in samples of a recording of n samples at `sr` Hz (si_quiet_runs' rows), -> the gaps
    to conceal, (first frame, frame count) pairs on the recording's 20 ms grid of n_rec_frames frames, sorted and disjoint: what
    normalize_gaps and plan_contexts accept as they are.  Integer arithmetic only (sr = 11025 has 220.5 samples per frame).
      cover   run [s, e) covers frames [s * 50 // sr - pad_frames, ceil(e * 50 / sr) + pad_frames), clamped to [0, n_rec_frames): every
              frame the run touches.  At 22 050 Hz this inverts `spans22`: a zeroed [441 p, 441 (p + l)) gives (p, l) back.
      edge    a run that touches sample 0 or sample n is leading or trailing padding, not a dropout, and a cover that does not fit the
              usable frames [0, lim_frames) cannot be served (lim_frames None: [0, n_rec_frames - 1), the encoder's frame count):
              skipped, reason "edge".
      merge   covers that overlap, touch or lie fewer than merge_frames frames apart become one gap.
      long    a merged gap of more than max_frames frames is skipped, reason "long".
    -> (gaps, skipped); skipped = (first frame, frame count, reason) per skipped run or merged gap, in order."""
    n, sr, n_rec, pad, mf, cap = int(n), int(sr), int(n_rec_frames), int(pad_frames), int(merge_frames), int(max_frames)
    if n < 0 or sr <= 0 or n_rec < 0 or pad < 0 or mf < 0 or cap < 1:
        raise ValueError(f"runs_to_gaps: n = {n}, sr = {sr}, n_rec_frames = {n_rec}, pad_frames = {pad}, merge_frames = {mf}, max_frames = {cap}")
    lim = max(n_rec - 1, 0) if lim_frames is None else min(int(lim_frames), n_rec)
    covers: List[Tuple[int, int]] = []
    skipped: List[Tuple[int, int, str]] = []
    for k, (s, l) in enumerate(sorted((int(s), int(l)) for s, l in runs)):
        e = s + l
        if l <= 0 or s < 0 or e > n:
            raise ValueError(f"runs_to_gaps: run {k} = samples [{s}, {e}) is not a run of a recording of {n} samples")
        a = min(max(s * 50 // sr - pad, 0), n_rec)
        b = min(max(-(-e * 50 // sr) + pad, 0), n_rec)
        if s == 0 or e == n or b > lim or b <= a:
            skipped.append((a, max(b - a, 0), "edge"))
        elif covers and a - covers[-1][1] < max(mf, 1):
            covers[-1] = (covers[-1][0], max(covers[-1][1], b))
        else:
            covers.append((a, b))
    gaps: List[Gap] = []
    for a, b in covers:
        if b - a > cap:
            skipped.append((a, b - a, "long"))
        else:
            gaps.append((a, b - a))
    return gaps, sorted(skipped)


# ---- repair at the file's own sample rate: gaps -> spans, regions and limits on the FILE's sample axis
RATE_MIN, RATE_MAX = 4000, 192000


def rate_ratio(sr: int) -> Tuple[int, int]:
    """(P, Q) = (22050, sr) / gcd: file sample i sits at position i * P / Q on the 22.05 kHz axis.  A ValueError for a rate outside
    [RATE_MIN, RATE_MAX]."""
    sr = int(sr)
    if not RATE_MIN <= sr <= RATE_MAX:
        raise ValueError(f"sample rate {sr} Hz is outside {RATE_MIN} .. {RATE_MAX}")
    g = math.gcd(22050, sr)
    return 22050 // g, sr // g


def rate_ratio16(sr: int) -> Tuple[int, int]:
    """(P16, Q16) = (16000, sr) / gcd: sample j of the recording's 16 kHz axis sits at file position j * Q16 / P16, and
    a file of n samples has ceil(n * P16 / Q16) samples on that axis.  (1, 1) for a 16 kHz file.  rate_ratio's ValueError."""
    sr = int(sr)
    rate_ratio(sr)
    g = math.gcd(16000, sr)
    return 16000 // g, sr // g


def file_fade(fade_ms: float, sr: int) -> int:
    """The cross-fade length in file samples: round(fade_ms * sr / 1000), Python's round (5 ms: 240 at 48 kHz, 220 at 44.1 kHz, 110 at
    22.05 kHz as config.patch_fade gives)."""
    return int(round(float(fade_ms) * int(sr) / 1000.0))


def invalid_ceiling(threshold: float) -> float:
    """The ceiling of kind "invalid"  from the `threshold` of find_gaps / conceal_*: 0, their default, is +inf (the
    samples that are not finite); anything else is the ceiling itself, in the file's own units.  A ValueError for a negative or NaN one."""
    t = float(threshold)
    if not t >= 0.0:
        raise ValueError(f"threshold = {threshold} with kind = 'invalid' is negative or NaN: the ceiling in the file's own units, or 0 for none")
    return math.inf if t == 0.0 else t


LEVEL_MAX_HALF = 1024   # SI_LEVEL_MAX_HALF of include/si_hip.h: the largest half window of the level detector


def level_half(win_ms: float, sr: int) -> int:
    """The level detector's half window in file samples: round(win_ms * sr / 2000), Python's round -- a window of 2 * half + 1 samples
    is win_ms long to within a sample (2 ms: 8 at 8 kHz, 22 at 22.05 kHz, 48 at 48 kHz, 192 at 192 kHz).  A ValueError that names the
    longest window this rate allows when half would pass LEVEL_MAX_HALF, and for a negative or NaN win_ms."""
    win_ms, sr = float(win_ms), int(sr)
    if not win_ms >= 0 or sr <= 0:
        raise ValueError(f"win_ms = {win_ms} at {sr} Hz: a window length in milliseconds, not negative")
    half = int(round(win_ms * sr / 2000.0)) if math.isfinite(win_ms) else LEVEL_MAX_HALF + 1
    if half > LEVEL_MAX_HALF:
        most = math.floor(2000.0 * LEVEL_MAX_HALF / sr * 1000.0) / 1000.0
        raise ValueError(f"win_ms = {win_ms} at {sr} Hz is a half window of more than {LEVEL_MAX_HALF} samples: at most win_ms = {most} at this rate")
    return half


# kind "impulse" (DESIGN.md 4.33): what find_gaps, conceal_* and `detect: {kind: impulse}` use when a key is not given.  Chosen on
# 22.05 kHz int16 speech; other rates, fp32 material and music are unmeasured.
IMPULSE_DEFAULTS = dict(order=16, win_ms=23.0, guard=4, pad=2, ratio=10.0)
IMPULSE_MAX_ORDER, IMPULSE_MAX_HALF, IMPULSE_MAX_GUARD, IMPULSE_MAX_PAD = 32, 1024, 64, 16   # SI_IMPULSE_MAX_* of include/si_hip.h


def check_impulse(who: str, order, half, guard, pad, ratio, rel_threshold=0.0, win_ms: Optional[float] = None, sr: Optional[int] = None) -> None:
    """What si_impulse_runs would refuse about its own arguments, as a ValueError that names the fix.  `half` is in samples; with win_ms
    and sr the message speaks of the window in milliseconds as well."""
    ints = {"order": order, "half": half, "guard": guard, "pad": pad}
    for k, v in ints.items():
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{who}: {k} = {v!r}: a whole number of samples" if k != "order" else f"{who}: order = {v!r}: a whole number")
    order, half, guard, pad = int(order), int(half), int(guard), int(pad)
    if not 2 <= order <= IMPULSE_MAX_ORDER:
        raise ValueError(f"{who}: order = {order}, outside 2 .. {IMPULSE_MAX_ORDER}: 16 is the default")
    if not 0 <= guard <= IMPULSE_MAX_GUARD:
        raise ValueError(f"{who}: guard = {guard} samples, outside 0 .. {IMPULSE_MAX_GUARD}: 4 is the default")
    if not 0 <= pad <= IMPULSE_MAX_PAD:
        raise ValueError(f"{who}: pad = {pad} samples, outside 0 .. {IMPULSE_MAX_PAD}: 2 is the default")
    at = f" (win_ms = {win_ms} at {sr} Hz)" if win_ms is not None and sr is not None else ""
    if half < guard + 1:
        need = f": raise win_ms to {2000.0 * (guard + 1) / sr:.3f} or more, or lower guard" if at else ": widen the window or lower guard"
        raise ValueError(f"{who}: half = {half} samples{at} is under guard + 1 = {guard + 1}: no sample would be left to compare with{need}")
    if half + pad > IMPULSE_MAX_HALF:
        need = f": lower win_ms to {math.floor(2000.0 * (IMPULSE_MAX_HALF - pad) / sr * 1000.0) / 1000.0} or less" if at else ""
        raise ValueError(f"{who}: half + pad = {half + pad} samples{at}, above {IMPULSE_MAX_HALF}{need}")
    if not 1.0 <= float(ratio) <= 1e6:
        raise ValueError(f"{who}: ratio = {ratio} is NaN or outside [1, 1e6]: how many times its neighbourhood's RMS prediction error a sample's "
                         f"must stand above; 10 is the default")
    if not 0.0 <= float(rel_threshold) <= 4.0:
        raise ValueError(f"{who}: rel_threshold = {rel_threshold} is NaN or outside [0, 4]: the floor under the prediction error as a fraction of the peak, "
                         f"0 for none")


def file_spans(gaps: Sequence[Gap], sr: int) -> List[Gap]:
    """(start, len) in FILE samples per gap (first frame, frame count) of the 20 ms grid: samples [ceil(p * sr / 50),
    ceil((p + l) * sr / 50)) -- exactly the file samples whose 22.05 kHz position lies in [441 p, 441 (p + l)).  Integers only."""
    sr = int(sr)
    return [(-(-int(p) * sr // 50), -(-(int(p) + int(l)) * sr // 50) - -(-int(p) * sr // 50)) for p, l in gaps]


def file_lim(lim22: int, sr: int, n_file: Optional[int] = None) -> int:
    """The first file sample whose 22.05 kHz position is at or past lim22: ceil(lim22 * Q / P), clamped to the file's n_file samples."""
    P, Q = rate_ratio(sr)
    lim = -(-int(lim22) * Q // P)
    return lim if n_file is None else min(lim, int(n_file))


def file_regions(spans_f: Sequence[Gap], lims_f: Sequence[int], fade_f: int) -> List[Optional[Gap]]:
    """`blend_regions` on the file axis: per (start, len) span and its lim_f the half-open range [max(s - fade_f, 0),
    min(s + l + fade_f, lim_f)) of file samples that are written; None for a span that starts at or past its lim_f."""
    fade_f = int(fade_f)
    return [None if l <= 0 or s >= lim else (max(s - fade_f, 0), min(s + l + fade_f, lim)) for (s, l), lim in zip(spans_f, lims_f)]


def rate_reach(nwin: int, step: int) -> int:
    """H: taps per wing of the band-limited interpolation, ceil(nwin / step) (audio.design_kaiser_best's table)."""
    return -(-int(nwin) // int(step))


def reach_regions22(regions_f: Sequence[Optional[Gap]], sr: int, reach: int, lo22: int, lim22: int) -> List[Optional[Gap]]:
    """File-axis regions -> the 22.05 kHz samples their interpolation reads: [floor(a * P / Q) - reach, floor((b - 1) * P / Q) + 1 +
    reach), clamped to [lo22, lim22) -- pass lo22 = 0 where the recording starts (taps before it read as zero) and lim22 = where the
    context's generated audio ends (taps at and past it read as zero).  The regions the generator windows must keep."""
    P, Q = rate_ratio(sr)
    out: List[Optional[Gap]] = []
    for reg in regions_f:
        if reg is None:
            out.append(None)
            continue
        a, b = int(reg[0]), int(reg[1])
        out.append((max(a * P // Q - int(reach), int(lo22)), min((b - 1) * P // Q + 1 + int(reach), int(lim22))))
    return out
