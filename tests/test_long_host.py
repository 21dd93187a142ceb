"""Recordings longer than one clip, host side: the planner that turns gaps on the recording's frame grid into context
clips, the chunk list of the region kernel, and the `long:` key of predict.yaml.  Pure Python, no GPU."""
import os

import numpy as np
import pytest

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd.config import load_predict_config

# the common shape of tests/test_gpu_long.py: a recording of 300 frames + 123 samples, clips of 75 frames (n22 = 33075, n16 = 24000,
# T = 74 encoder frames, Tm = 75 mel frames: 74 usable), 15 frames of context on each side
N_REC, CLIP, CTX, LIM = 300, 75, 15, 74
GAPS = [(2, 3), (100, 5), (106, 4), (140, 6), (292, 5)]


def _plan(gaps=GAPS, n_rec=N_REC, **kw):
    kw = {"clip_frames": CLIP, "min_context": CTX, "lim_frames": LIM, **kw}
    return G.plan_contexts(gaps, n_rec, **kw)


def test_plan_contexts_written_out_by_hand():
    """budget = 75 - 2 * 15 = 45 frames.  (2, 3) alone: centre (2 + 5) // 2 - 37 = -34 -> clamped to 0.  (100, 5) takes (106, 4) (end 110
    - 100 = 10 <= 45) and not (140, 6) (146 - 100 = 46 > 45): centre (100 + 110) // 2 - 37 = 68, usable frames [68, 142) cut (140, 6)
    to two frames.  (140, 6): centre (140 + 146) // 2 - 37 = 106, usable [106, 180) hold (106, 4) whole at local frame 0 and miss
    (100, 5), which ends at 105.  (292, 5): centre 294 - 37 = 257 -> clamped to 300 - 75 = 225."""
    want = [{"start": 0, "frames": 75, "own": [(2, 3)], "own_index": [0], "foreign": []},
            {"start": 68, "frames": 75, "own": [(32, 5), (38, 4)], "own_index": [1, 2], "foreign": [(72, 2)]},
            {"start": 106, "frames": 75, "own": [(34, 6)], "own_index": [3], "foreign": [(0, 4)]},
            {"start": 225, "frames": 75, "own": [(67, 5)], "own_index": [4], "foreign": []}]
    assert _plan() == want
    assert _plan(list(reversed(GAPS))) == want                       # the gaps are sorted first
    assert _plan([]) == []
    # without lim_frames every frame of the clip is usable: the cut foreign gap keeps three frames
    assert G.plan_contexts(GAPS, N_REC, CLIP, CTX)[1]["foreign"] == [(72, 3)]


def test_every_gap_is_owned_once_and_has_its_context():
    """Random gap sets: each gap is own in exactly one context, lies min_context frames from that context's edges unless the context
    is clamped at an end of the recording, and every other gap that meets the context's usable frames is foreign, clipped."""
    rng = np.random.default_rng(5)
    for trial in range(40):
        n_rec = int(rng.integers(400, 3000))
        starts = np.sort(rng.choice(np.arange(0, n_rec - 12, 12), size=int(rng.integers(1, 25)), replace=False))
        gaps = [(int(s), int(rng.integers(1, 9))) for s in starts]    # at least 3 frames apart
        plan = G.plan_contexts(gaps, n_rec, 200, 50, lim_frames=199)
        owned = sorted(k for c in plan for k in c["own_index"])
        assert owned == list(range(len(gaps)))
        for c in plan:
            f = c["start"]
            assert 0 <= f <= n_rec - 200 and len(c["own"]) + len(c["foreign"]) <= G.MAX_SPANS
            for (p, l), k in zip(c["own"], c["own_index"]):
                assert (p + f, l) == gaps[k] and 0 <= p and p + l <= 199
                assert p >= 50 or f == 0
                assert p + l <= 150 or f == n_rec - 200
            want = [(max(p, f) - f, min(p + l, f + 199) - max(p, f)) for k, (p, l) in enumerate(gaps)
                    if k not in c["own_index"] and max(p, f) < min(p + l, f + 199)]
            assert c["foreign"] == want


def test_recording_shorter_than_a_clip_is_one_context():
    plan = _plan([(40, 5), (3, 2), (60, 4)], n_rec=70, lim_frames=69)
    assert plan == [{"start": 0, "frames": 70, "own": [(3, 2), (40, 5), (60, 4)], "own_index": [0, 1, 2], "foreign": []}]
    # exactly one clip: still one context, though first start and last end are more than the budget apart
    plan = _plan([(3, 2), (60, 4)], n_rec=75)
    assert len(plan) == 1 and plan[0]["start"] == 0 and plan[0]["frames"] == 75 and plan[0]["own"] == [(3, 2), (60, 4)]
    with pytest.raises(ValueError, match=r"\[69, 70\) does not fit the usable frames \[0, 69\)"):
        _plan([(69, 1)], n_rec=70, lim_frames=69)


def test_plan_contexts_refuses():
    with pytest.raises(ValueError, match=r"gap 0 = frames \[100, 146\) is longer than the 45 frames"):
        _plan([(100, 46)])
    assert len(_plan([(100, 45)])) == 1                                  # the budget itself fits
    with pytest.raises(ValueError, match=r"gap 0 = frames \[299, 300\) does not fit the usable frames \[225, 299\)"):
        _plan([(299, 1)])                                                # the recording's last frame: the encoder has no such frame
    with pytest.raises(ValueError, match=r"gap 1 = frames \[298, 301\) does not fit the recording \(300 frames\)"):
        _plan([(10, 2), (298, 3)])
    with pytest.raises(ValueError, match="does not fit the recording"):
        _plan([(-1, 2)])
    with pytest.raises(ValueError, match=r"gap 1 = frames \[104, 107\) overlaps gap 0 = \[100, 105\)"):
        _plan([(104, 3), (100, 5)])
    assert len(_plan([(100, 5), (105, 3)])) == 1                         # touching gaps are fine
    with pytest.raises(ValueError, match=r"gap 1 = \(50, 0\) has no frames"):
        _plan([(10, 2), (50, 0)])
    with pytest.raises(ValueError, match=r"gap 1 = \(7,\) is not a \(first frame, frame count\) pair"):
        _plan([(10, 2), (7,)])
    with pytest.raises(ValueError, match="is not a"):
        _plan([(10, 2), "ab"])
    # 17 gaps two frames apart span 33 frames <= 45: the group closes at MAX_SPANS = 16 and the 17th gap, one frame after the 16th,
    # goes to another context -- closer than two cross-fades
    dense = [(100 + 2 * i, 1) for i in range(17)]
    with pytest.raises(ValueError, match=r"gap 16 = frames \[132, 133\) lies 1 frames after gap 15, which another context serves"):
        _plan(dense)
    # ... and three frames apart the groups are legal, but the first context holds its 16 gaps and the 17th as a foreign one
    dense = [(100 + 2 * i, 1) for i in range(16)] + [(134, 1)]
    with pytest.raises(ValueError, match=r"the context of gap 0 = frames \[100, 101\) holds 16 gaps of its own and 1 of other contexts"):
        _plan(dense)
    # cross-context ramp overlap: (100, 5) .. (140, 5) is 45 frames, (146, 3) starts one frame after it and does not fit the group
    with pytest.raises(ValueError, match=r"gap 2 = frames \[146, 149\) lies 1 frames after gap 1"):
        _plan([(100, 5), (140, 5), (146, 3)])
    assert len(_plan([(100, 5), (140, 5), (147, 3)])) == 2              # two frames = one cross-fade each side
    with pytest.raises(ValueError, match=r"lies 3 frames after gap 1.*2 frames each side"):
        _plan([(100, 5), (140, 5), (148, 3)], fade_frames=2)
    with pytest.raises(ValueError, match="longer than two contexts"):
        _plan(clip_frames=30)


def test_own_spans_shifted_back_are_the_recordings_spans():
    """spans22 gives p * 441 and spans16 p * 320 + 80, so the local span tables of a context that starts at frame f are the
    recording's, shifted by 441 f and 320 f."""
    rec22, rec16 = G.spans22([GAPS])[0], G.spans16([GAPS])[0]
    assert rec22 == [(441 * p, 441 * l) for p, l in GAPS]
    for c in _plan():
        f = c["start"]
        loc22, loc16 = G.spans22([c["own"]], [CLIP * 441])[0], G.spans16([c["own"]])[0]
        for k, (s22, l22), (s16, l16) in zip(c["own_index"], loc22, loc16):
            assert (s22 + 441 * f, l22) == rec22[k] and (s16 + 320 * f, l16) == rec16[k]


@pytest.mark.parametrize("fade", [0, 110, 300])
def test_region_chunks_against_a_per_sample_scan(fade):
    chunk = G.PC_CHUNK
    assert chunk == 2048
    spans = [(2 * chunk + fade, 300), (2 * chunk + fade + 300 + 2 * fade, chunk), (5 * chunk - 10, 20), (5 * chunk + 10 + 2 * fade, 3),
             (9 * chunk + fade, chunk - 2 * fade), (20 * chunk - 5, 3 * chunk)]
    n = 24 * chunk + 77
    regions = [(max(s - fade, 0), min(s + l + fade, n)) for s, l in spans]
    got = G.region_chunks(regions)
    touched = np.zeros((len(regions), -(-n // chunk)), dtype=bool)
    for k, (a, b) in enumerate(regions):
        for m in range(a, b):
            touched[k, m // chunk] = True
    want = []
    for c in np.flatnonzero(touched.any(axis=0)):
        ks = np.flatnonzero(touched[:, c])
        assert np.array_equal(ks, np.arange(ks[0], ks[-1] + 1))
        want.append((int(c), int(ks[0]), int(ks[-1]) + 1))
    assert got == want
    assert [c for c, _, _ in got] == sorted({c for c, _, _ in got})
    assert any(k1 - k0 > 1 for _, k0, k1 in got)                        # a chunk that two regions share
    assert (9, 4, 5) in got and all(c != 10 for c, _, _ in got)         # a region that ends on a chunk's last sample
    assert G.region_chunks([]) == []
    with pytest.raises(ValueError, match="not sorted"):
        G.region_chunks([(5000, 6000), (100, 200)])
    with pytest.raises(ValueError, match="empty"):
        G.region_chunks([(100, 100)])


def _yaml(tmp_path, extra):
    src = open(os.path.join(os.path.dirname(__file__), "golden", "iea_predict.yaml")).read()
    p = tmp_path / "predict.yaml"
    p.write_text(src + "\n" + extra)
    return str(p)


def test_predict_yaml_long_key(tmp_path):
    assert load_predict_config(_yaml(tmp_path, "")).long is None
    assert load_predict_config(_yaml(tmp_path, "long: {}\n")).long == {"clip_s": 4.0, "context_s": 1.0, "batch": 32}
    assert load_predict_config(_yaml(tmp_path, "long:\n")).long == {"clip_s": 4.0, "context_s": 1.0, "batch": 32}
    cfg = load_predict_config(_yaml(tmp_path, "long:\n  clip_s: 1.5\n  context_s: 0.3\n  batch: 8\npatch:\n  fade_ms: 0\n"))
    assert cfg.long == {"clip_s": 1.5, "context_s": 0.3, "batch": 8} and cfg.patch_fade == 0
    with pytest.raises(ValueError, match="unknown key `clip_frames` in `long:`"):
        load_predict_config(_yaml(tmp_path, "long:\n  clip_frames: 200\n"))
    with pytest.raises(ValueError, match="long.context_s = -1.0 is negative"):
        load_predict_config(_yaml(tmp_path, "long:\n  context_s: -1\n"))
    with pytest.raises(ValueError, match="long.batch = -2 is negative"):
        load_predict_config(_yaml(tmp_path, "long:\n  batch: -2\n"))
    with pytest.raises(ValueError, match="mapping"):
        load_predict_config(_yaml(tmp_path, "long: 4\n"))
    with pytest.raises(ValueError, match="clip_s > 2 \\* context_s"):
        load_predict_config(_yaml(tmp_path, "long:\n  clip_s: 2\n"))
    with pytest.raises(ValueError, match="batch >= 1"):
        load_predict_config(_yaml(tmp_path, "long:\n  batch: 0\n"))
