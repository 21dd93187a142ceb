"""The keyword space of engine.conceal_file as a covering set of calls: the factors and their levels, the combinations the
engine refuses, a deterministic all-pairs generator, one damaged file per case and, from the float64 references alone, what the call
must return.  Pure Python and numpy; importing it and everything in it needs no GPU.

conceal_file is documented as a composition of public calls -- find_gaps -> (mend_runs on a copy) -> gaps.runs_to_gaps -> patch_file --
and each of those is pinned on its own.  What is not pinned is the glue between two keywords that no route test ran together.  Pairs can
be enumerated: every pair of levels the refusals allow occurs in at least one case of `covering_set()`.

FACTORS, one row per keyword (or group of keywords that only make sense together):

    kind     quiet, held, any, level, burst, invalid, impulse
    stype    fp32, int16, s24 (packed 24-bit)
    layout   mono (n,); one (n, 1); each2 (n, 2) detect="each"; joint2 (n, 2) detect="joint"; each3 (n, 3) detect="each", channel 1 clean
    sr       8000, 16000, 22050, 44100, 48000
    feed     recording, contexts
    clips16  resampled, file
    mend     off; on (min_ms=0, mend_ms=1.0; mend_order / mend_context at their defaults (32, 512) where the two contexts, 1024
             samples, span less than 50 ms of the file -- sr >= 22050 --, and (8, 64) at 8 and 16 kHz)
    rel      0; above 0 (per kind: REL)
    batch    32; 2
    input    host (a CPU tensor); device

CONSTRAINTS restates the refusals of engine.py, each with the function and the text it raises; `refused(case)` names the first one a
case runs into, None for a case the engine serves."""
import functools
import itertools

import numpy as np

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd.arch import HubertArch, mel_frames
from tests import burst_ref as B
from tests import channels_ref as CH
from tests import dead_ref as R
from tests import detect_ref as D
from tests import impulse_ref as I
from tests import invalid_ref as V
from tests import level_ref as L
from tests import mend_ref as M
from tests import s24_ref as S

FACTORS = (
    ("kind", ("quiet", "held", "any", "level", "burst", "invalid", "impulse")),
    ("stype", ("fp32", "int16", "s24")),
    ("layout", ("mono", "one", "each2", "joint2", "each3")),
    ("sr", (8000, 16000, 22050, 44100, 48000)),
    ("feed", ("recording", "contexts")),
    ("clips16", ("resampled", "file")),
    ("mend", ("off", "on")),
    ("rel", (0, 1)),
    ("batch", (32, 2)),
    ("input", ("host", "device")),
)
NAMES = tuple(name for name, _ in FACTORS)
SEED = 1
MAX_CASES = 64
MAX_SEEDS = 8

# name -> (where engine.py refuses it, a regular expression of the text).  The first five bind two factors of the table
# (TABLE_CONSTRAINTS); the others bind a keyword the table fixes per kind.  Each is held by one forbidden call (FORBIDDEN).
CONSTRAINTS = {
    "s24_feed": ("conceal_file, `if s24 and feed != \"contexts\"`", r"conceal_file: packed 24-bit PCM needs feed = 'contexts'"),
    "s24_22050": ("conceal_file, `if s24 and sr == 22050`", r"conceal_file: packed 24-bit PCM at 22050 Hz is not served"),
    "clips16_feed": ("patch_file / _patch_file_channels, `if clips16 == \"file\" and feed != \"contexts\"`, behind the sr == 22050 return: a "
                     "22.05 kHz file reads neither keyword", r"patch_file: clips16 = 'file' needs feed = 'contexts'"),
    "invalid_feed": ("patch_file, `if ceiling is not None and sr != 22050 and feed != \"contexts\"`", r"patch_file: ceiling = \S+ needs feed=\"contexts\" at \d+ Hz"),
    "invalid_rel": ("find_gaps, kind == \"invalid\": `if float(rel_threshold) != 0.0`", r"find_gaps: rel_threshold = \S+ with kind = 'invalid'"),
    "invalid_held_tol": ("find_gaps, kind == \"invalid\": `if float(held_tol) != 0.0`", r"find_gaps: held_tol = \S+ with kind = 'invalid'"),
    "held_tol_kind": ("find_gaps, kinds level / burst / impulse: `if float(held_tol) != 0.0`", r"find_gaps: held_tol = \S+ with kind = '(level|burst|impulse)'"),
    "burst_zero": ("find_gaps, kind == \"burst\": `if float(threshold) == 0.0 and float(rel_threshold) == 0.0`", r"find_gaps: kind = 'burst' with threshold = 0 and rel_threshold = 0"),
    "win_ms_rate": ("gaps.level_half (kinds level, burst) and gaps.check_impulse (kind impulse), called by find_gaps",
                    r"win_ms = \S+ at \d+ Hz is a half window of more than 1024 samples|half \+ pad = \d+ samples \(win_ms = \S+ at \d+ Hz\), above 1024"),
    "mend_len": ("conceal_file, `if mend_len > native.MEND_MAX_LEN` / `if mend_len < 1`", r"conceal_file: mend_ms = \S+ at \d+ Hz is (max_len = \d+ samples, at most 64|less than one sample)"),
}
TABLE_CONSTRAINTS = ("s24_feed", "s24_22050", "clips16_feed", "invalid_feed", "invalid_rel")

CLIP, CTX, FRAMES, TAIL = 75, 15, 130, 77              # clip_frames, min_context; the file: 130 frames of 20 ms and an odd tail
CHANNELS = {"mono": 1, "one": 1, "each2": 2, "joint2": 2, "each3": 3}
DTYPE = {"fp32": np.float32, "int16": np.int16, "s24": M.S24}
FULL = {"fp32": 1.0, "int16": 32768.0, "s24": 8388608.0}
REL = {"quiet": 2.0 ** -9, "held": 2.0 ** -9, "any": 2.0 ** -9, "level": 2.0 ** -9, "burst": 1.2, "impulse": 2.0 ** -6,
       "invalid": 0.5}                                 # refused: what a refused call would carry
FLOOR = 328                                            # int16 steps: no clean sample is quieter (0.01 of full scale)
NAN_PAYLOAD = 0x7FC00001


# ------------------------------------------------------------------------------------------------------------ the cases
def refused(case):
    """The first constraint of the table a case runs into, in the order the engine meets them; None when it is served."""
    s24 = case["stype"] == "s24"
    if s24 and case["feed"] != "contexts":
        return "s24_feed"
    if s24 and case["sr"] == 22050:
        return "s24_22050"
    if case["kind"] == "invalid" and case["sr"] != 22050 and case["feed"] != "contexts":
        return "invalid_feed"
    if case["clips16"] == "file" and case["feed"] != "contexts" and case["sr"] != 22050:
        return "clips16_feed"
    if case["kind"] == "invalid" and case["rel"]:
        return "invalid_rel"
    return None


# One call per constraint that the engine must refuse before it launches anything: name -> (sample type, sr, conceal_file's keywords).
FORBIDDEN = {
    "s24_feed": ("s24", 48000, dict(feed="recording")),
    "s24_22050": ("s24", 22050, dict(feed="contexts")),
    "clips16_feed": ("fp32", 48000, dict(feed="recording", clips16="file")),
    "invalid_feed": ("fp32", 48000, dict(kind="invalid", min_ms=0, feed="recording")),
    "invalid_rel": ("fp32", 48000, dict(kind="invalid", min_ms=0, feed="contexts", rel_threshold=0.5)),
    "invalid_held_tol": ("fp32", 48000, dict(kind="invalid", min_ms=0, feed="contexts", held_tol=1.0)),
    "held_tol_kind": ("int16", 16000, dict(kind="level", threshold=16.0, held_tol=1.0)),
    "burst_zero": ("int16", 16000, dict(kind="burst", threshold=0.0)),
    "win_ms_rate": ("fp32", 48000, dict(kind="level", threshold=2.0 ** -11, win_ms=50.0)),
    "mend_len": ("fp32", 48000, dict(kind="invalid", min_ms=0, feed="contexts", mend_ms=2.0)),
}


def forbidden_file(stype, sr):
    """One second of a constant, as a host tensor in the sample type's own form."""
    import torch
    if stype == "s24":
        return torch.from_numpy(S.pack(np.full(sr, 1000, M.S24)))
    return torch.full((sr,), 0.1) if stype == "fp32" else torch.full((sr,), 1000, dtype=torch.int16)


def product():
    """Every combination of levels, served or refused, as dictionaries in the table's order."""
    return [dict(zip(NAMES, values)) for values in itertools.product(*(levels for _, levels in FACTORS))]


def pairs_of(case):
    """The 45 (factor, level, factor, level) pairs of one case."""
    return [(a, case[a], b, case[b]) for a, b in itertools.combinations(NAMES, 2)]


@functools.lru_cache(maxsize=None)
def covering_set(seed=SEED):
    """A list of served cases in which every pair of levels that some served case holds occurs at least once.  Greedy: the served cases
    are shuffled once by `seed`, and the case that covers the most pairs not yet covered is taken -- the first such in the shuffled order
    -- until none is left.  No other randomness."""
    served = [c for c in product() if refused(c) is None]
    order = np.random.default_rng(seed).permutation(len(served))
    served = [served[i] for i in order]
    index = {}
    table = np.empty((len(served), len(NAMES) * (len(NAMES) - 1) // 2), np.int64)
    for i, c in enumerate(served):
        for j, p in enumerate(pairs_of(c)):
            table[i, j] = index.setdefault(p, len(index))
    open_ = np.ones(len(index), bool)
    chosen = []
    while open_.any():
        gain = open_[table].sum(axis=1)
        best = int(np.argmax(gain))
        chosen.append(served[best])
        open_[table[best]] = False
    return tuple(case_id(c) for c in chosen), tuple(chosen)


def case_id(case):
    return "-".join(f"{'rel' if k == 'rel' else 'b' if k == 'batch' else 'mend' if k == 'mend' else ''}{case[k]}" for k in NAMES)


def detect_of(case):
    return {"each2": "each", "each3": "each", "joint2": "joint"}.get(case["layout"])


def mend_limits(case):
    """(max_len, order, context) of a case with mend on."""
    sr = case["sr"]
    order, context = (32, 512) if 2 * 512 * 1000 < 50 * sr else (8, 64)
    return int(round(1.0 * sr / 1000.0)), order, context


def threshold_of(case):
    """`threshold` in the file's own units, exactly as the call gets it (an fp32 value: the device holds it in fp32)."""
    fs = FULL[case["stype"]]
    frac = {"quiet": 0.0, "held": 0.0, "any": 0.0, "level": 2.0 ** -11, "burst": 1.15, "invalid": 0.95, "impulse": 0.0}[case["kind"]]
    return float(np.float32(frac * fs))


def win_ms_of(case):
    """level: 0.75 ms, so that a stretch of max_len samples still holds a whole window (2 half + 1 <= max_len at every rate); burst:
    half = 1, so that one garbage sample is a run of at most 6; impulse: the default."""
    return {"level": 0.75, "burst": 2000.0 / case["sr"]}.get(case["kind"])


def keywords(case):
    """conceal_file's keywords for a case (x and sr are positional)."""
    kw = dict(threshold=threshold_of(case), clip_frames=CLIP, min_context=CTX, batch=case["batch"], feed=case["feed"], clips16=case["clips16"],
              kind=case["kind"])
    if detect_of(case):
        kw["detect"] = detect_of(case)
    if case["rel"]:
        kw["rel_threshold"] = REL[case["kind"]]
    if win_ms_of(case) is not None:
        kw["win_ms"] = win_ms_of(case)
    if case["clips16"] == "file" and case["feed"] == "contexts" and case["sr"] != 22050:
        kw["return_windows"] = True                                     # where clips16 is read: the passes carry the 16 kHz clips it made
    if case["mend"] == "on":
        _, order, context = mend_limits(case)
        kw.update(min_ms=0.0, mend_ms=1.0, mend_order=order, mend_context=context)
    elif case["kind"] in ("invalid", "impulse"):
        kw["min_ms"] = 0.0                                              # as the docstring asks: a single NaN, a click, is a run of a few samples
    return kw


# ------------------------------------------------------------------------------------------------------------ the file
def _clean(sr, n, seed):
    """Speech on the int16 grid with no sample under FLOOR steps and no two equal neighbours: nothing in it is quiet or held."""
    import torch                                                       # synth is torch code; nothing here touches a device
    from speech_inpainting_amd import synth
    q = np.rint(synth.synth_wave(1, n, seed, sr=sr)[0].to(torch.float64).numpy() * 32767.0).astype(np.int64)
    q = np.where(np.abs(q) < FLOOR, np.where(q < 0, -FLOOR, FLOOR), q)
    for _ in range(64):
        same = np.flatnonzero(q[1:] == q[:-1]) + 1
        if same.size == 0:
            break
        q[same] += np.where(q[same] > 0, 1, -1)
    assert not np.any(q[1:] == q[:-1]) and np.abs(q).min() >= FLOOR and np.abs(q).max() < 16384
    return q


def _typed(q, stype, rng):
    if stype == "fp32":
        return (q / 32768.0).astype(np.float32)                         # exact: 15 bits x 2^-15
    if stype == "int16":
        return q.astype(np.int16)
    return (q * 256 + rng.integers(0, 256, q.size)).astype(M.S24)


def _plant(col, case, rng, shift, extra=False):
    """The defects of the case's kind in one channel, `shift` frames later than in channel 0.  Three short ones -- the second across a
    2048-sample seam -- and three blocks of 120, 100 and 140 ms (for kind "impulse", which finds no block: two clicks 40 samples apart,
    which mend_runs leaves as NEAR).  extra: one more defect at frames 120 .. 124, which joint detection must not see."""
    sr, kind, stype = case["sr"], case["kind"], case["stype"]
    per, fs, n = sr // 50, FULL[stype], col.size
    ml = int(round(sr / 1000.0))
    top = fs - 1.0 if stype != "fp32" else 1.0
    s1, s3 = (8 + shift) * per + 37, (78 + shift) * per + per // 2 + 5
    s2 = 2048 * int(round((38 + shift) * per / 2048.0)) - 1
    # the blocks start 42 frames apart: no clip of CLIP frames holds two of them with CTX frames of context on either side
    blocks = [((16 + shift) * per + 13, 6 * per - 29), ((58 + shift) * per + 13, 5 * per - 29), ((100 + shift) * per + 13, 7 * per - 29)]
    far = (120 * per + 13, 4 * per - 29)
    val = (lambda f: np.float32(f)) if stype == "fp32" else (lambda f: int(round(f * top)))

    def zeros(s, m):
        col[s:s + m] = 0

    def held(s, m):
        c = val(0.05)
        col[s:s + m] = c
        for t in (s - 1, s + m):
            if col[t] == c:
                col[t] = val(0.06)

    def floor_noise(s, m):
        v = rng.integers(1, 4, m) * rng.choice([-1, 1], m)
        col[s:s + m] = (v / 32768.0).astype(np.float32) if stype == "fp32" else v if stype == "int16" else v * 256

    def garbage(s, m):
        sign = -1.0 if float(col[s]) > 0 else 1.0                       # against the speech: the second difference adds up
        g = rng.uniform(0.96, 0.999, m) * sign * (-1.0) ** np.arange(m)
        col[s:s + m] = g.astype(np.float32) if stype == "fp32" else np.rint(g * top).astype(col.dtype)

    def nan(s, m):
        col[s:s + m] = V.bits([NAN_PAYLOAD])[0]

    def infs(s, m):
        col[s:s + m] = [(np.inf, -np.inf, V.bits([NAN_PAYLOAD])[0])[k % 3] for k in range(m)]

    def clicks(s, m):
        I.plant(col, s, amp=0.7, width=m)

    def near_pair(s, m):
        I.plant(col, s, amp=0.7, width=1)
        I.plant(col, s + 40, amp=0.7, width=2, sign=-1)

    fp = stype == "fp32"
    plan = {
        "quiet": ([(zeros, 1), (zeros, 3), (zeros, min(8, ml))], [zeros, zeros, zeros]),
        "held": ([(held, 2), (held, 3), (held, min(8, ml))], [held, held, held]),
        "any": ([(zeros, 1), (zeros, 3), (held, min(8, ml))], [zeros, held, zeros]),
        "level": ([(floor_noise, ml), (floor_noise, ml - 1), (floor_noise, ml)], [floor_noise, floor_noise, floor_noise]),
        "burst": ([(garbage, 1), (garbage, 2), (garbage, 1)], [garbage, garbage, garbage]),
        "invalid": ([(nan if fp else garbage, 1), (infs if fp else garbage, 3), (garbage, min(8, ml))], [nan if fp else garbage, garbage, garbage]),
        "impulse": ([(clicks, 1), (clicks, 2), (clicks, 3)], [near_pair, near_pair, near_pair]),
    }[kind]
    if extra:
        plan[1][0](*far)
    for (fn, m), s in zip(plan[0], (s1, s2, s3)):
        fn(s, m)
    for fn, (s, m) in zip(plan[1], blocks):
        fn(s, m)


def build_file(case, seed):
    """The case's file in the references' dtype (float32, int16, or int32 values of 24 bits), shaped as the layout says."""
    sr, layout = case["sr"], case["layout"]
    n = FRAMES * (sr // 50) + TAIL
    rng = np.random.default_rng(1000 * seed + 7)
    cols = []
    for c in range(CHANNELS[layout]):
        col = _typed(_clean(sr, n, 16 * seed + 3 + c), case["stype"], rng)
        if layout == "joint2":
            _plant(col, case, rng, 0, extra=(c == 0))
        elif not (layout == "each3" and c == 1):
            _plant(col, case, rng, 0 if c == 0 else 3)
        cols.append(col)
    if layout == "mono":
        return cols[0]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def as_input(x, case, device=None):
    """The file as conceal_file takes it: a torch tensor, packed bytes for 24-bit, on `device` for input = "device"."""
    import torch
    t = torch.from_numpy(S.pack(x) if case["stype"] == "s24" else np.ascontiguousarray(x))
    return t.to(device) if (case["input"] == "device" and device is not None) else t


# ------------------------------------------------------------------------------------------------------------ the expectation
class Undecided(Exception):
    """A windowed reference has a decision within an addition order of its limit: the file is rebuilt from the next seed."""


def _rows(x, case, channel, min_len):
    """(rows, T or None) of one detection from the float64 reference of the case's kind.  x (n,) with channel None, or (n, ch)."""
    kind, thr, rel = case["kind"], threshold_of(case), (REL[case["kind"]] if case["rel"] else 0.0)
    sr = case["sr"]
    if kind == "quiet" and not rel:
        if x.ndim == 1:
            return D.quiet_runs_ref(x, thr, min_len), None
        return (CH.joint_runs_ref(x, thr, min_len) if channel < 0 else D.quiet_runs_ref(x[:, channel], thr, min_len)), None
    if kind in ("quiet", "held", "any"):
        code = {"quiet": R.QUIET, "held": R.HELD, "any": R.ANY}[kind]
        return R.dead_runs_ref(x, code, thr, rel, 0.0, min_len, channel), float(R.threshold_ref(x, thr, rel, channel))
    if kind == "invalid":
        return V.invalid_runs_ref(x, thr, min_len, channel), thr
    if kind in ("level", "burst"):
        undecided = []
        mask = (L.level_mask if kind == "level" else B.burst_mask)(x, G.level_half(win_ms_of(case), sr), thr, rel, channel, report=undecided)
        if undecided:
            raise Undecided(f"{kind}: samples {undecided[:4]}")
        return R.runs_of(mask, min_len), float(R.threshold_ref(x, thr, rel, channel))
    d = G.IMPULSE_DEFAULTS
    kw = dict(order=d["order"], half=G.level_half(d["win_ms"], sr), guard=d["guard"], pad=d["pad"], ratio=d["ratio"], thr=thr, rel=rel,
              channel=channel, min_len=min_len)
    try:
        rows, T, _ = I.check(I.Case(case_id(case), x, kw))
    except AssertionError as e:
        raise Undecided(f"impulse: {e}")
    return rows, float(T)


def recording_frames(n, sr):
    """(n_rec, lim) of a file of n samples: the frames of its 22.05 kHz length ceil(n 22050 / sr), and the usable ones, as
    engine.recording_frames documents them (the last context's min(T, Tm), counted from where it starts)."""
    P, Q = G.rate_ratio(sr)
    n22 = -(-n * P // Q)
    n_rec = n22 // 441
    whole = n_rec <= CLIP
    L22 = n22 if whole else CLIP * 441
    L16 = -(-L22 * 16000 // 22050)
    lim = min(HubertArch.tiny().num_frames(L16), mel_frames(L22))
    return n_rec, max(lim, 0) + (0 if whole else n_rec - CLIP)


def _joint_status(col):
    """conceal_file's documented joint status: AR or LINE when every channel filled the row (LINE if any did by the line), else the
    first channel's status that is no fill."""
    bad = [v for v in col if v not in (M.AR, M.LINE)]
    return bad[0] if bad else M.LINE if M.LINE in col else M.AR


def _expect(case, x):
    sr, layout = case["sr"], case["layout"]
    ch, n = CHANNELS[layout], x.shape[0]
    many, each = ch >= 2, detect_of(case) == "each"
    flat = x if many else x.reshape(-1)
    kw = keywords(case)
    min_len = max(1, int(round(kw.get("min_ms", 5.0) * sr / 1000.0)))
    n_rec, lim = recording_frames(n, sr)
    max_ms = min(400.0, 20.0 * (CLIP - 2 * CTX)) if n_rec > CLIP else 400.0
    P, Q = G.rate_ratio(sr)
    fade22 = -(-G.file_fade(5.0, sr) * P // Q)
    mf = 2 * max(-(-fade22 // 441), 1)                                   # merge_frames None: twice the frames one cross-fade reaches over
    to_gaps = lambda rows: G.runs_to_gaps(rows, n, sr, n_rec, lim, 0, mf, max(int(max_ms // 20), 1))
    channels = list(range(ch)) if (many and each) else [-1 if many else None]
    found = [_rows(flat, case, c, min_len) for c in channels]
    rows = [[(int(s), int(l)) for s, l in r.tolist()] for r, _ in found]
    T = [t for _, t in found]
    out = {"x": x, "rows": rows if (many and each) else rows[0], "kw": kw, "mend": []}
    if T[0] is not None:
        out["threshold"] = T if (many and each) else T[0]
    if case["mend"] == "on":
        max_len, order, context = mend_limits(case)
        mended, left = [], []
        for k, c in enumerate(channels):
            mend_in = list(range(ch)) if c == -1 else [c]               # joint: every channel, in channel order
            results = [M.mend(flat, rows[k], max_len, order, context, channel=m) if rows[k] else None for m in mend_in]
            status = [_joint_status([int(r.status[i]) for r in results]) for i in range(len(rows[k]))]
            mended.append([(s, l, st) for (s, l), st in zip(rows[k], status) if l <= max_len])
            left.append([r for r, st in zip(rows[k], status) if st not in (M.AR, M.LINE)])
            out["mend"] += [(m, rows[k], r) for m, r in zip(mend_in, results) if r is not None]
        out["mended"] = mended if (many and each) else mended[0]
    else:
        left = rows
    mapped = [to_gaps(r) for r in left]
    out["gaps"] = [g for g, _ in mapped] if (many and each) else mapped[0][0]
    out["skipped"] = [k for _, k in mapped] if (many and each) else mapped[0][1]
    return out


_EXPECTED = {}


def expected(case):
    """-> the dictionary of what conceal_file must return for the case, from the references alone: x (the file), kw (the keywords), rows,
    gaps, skipped [, threshold] [, mended], per channel where the route returns them per channel; mend: (channel, rows, tests/mend_ref.py
    Result) per mended channel.  The file is the first of MAX_SEEDS seeds at which every windowed reference decides; none is an error."""
    key = case_id(case)
    if key not in _EXPECTED:
        why = []
        for seed in range(MAX_SEEDS):
            try:
                _EXPECTED[key] = dict(_expect(case, build_file(case, seed)), seed=seed)
                break
            except Undecided as e:
                why.append(str(e))
        else:
            raise AssertionError(f"{key}: no seed of 0 .. {MAX_SEEDS - 1} gives a file that every reference decides: {why}")
    return _EXPECTED[key]


def blend_set(n, gaps, sr, fade_ms=5.0):
    """The file samples patch_file may change for `gaps`: their spans widened by the file-rate fade on either side."""
    some = np.zeros(n, bool)
    fade = G.file_fade(fade_ms, sr)
    for s, l in G.file_spans(gaps, sr):
        some[max(s - fade, 0):s + l + fade] = True
    return some
