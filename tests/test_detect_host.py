"""Dropout detection, host side: the numpy reference the GPU tests compare against, gaps.runs_to_gaps (sample runs at
any file rate -> planner-safe gaps on the 20 ms grid), the `detect:` key of predict.yaml, and the ABI's declaration.  No GPU."""
import os

import numpy as np
import pytest
import yaml

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd.config import load_predict_config
from tests import detect_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REC, CLIP, CTX, LIM = 300, 75, 15, 74           # the geometry of tests/test_gpu_long.py
N22 = N_REC * 441 + 123
GAPS = [(2, 3), (100, 5), (106, 4), (140, 6), (292, 5)]


# ------------------------------------------------------------------------------------------------------------ the reference
def test_the_reference_against_runs_written_out_by_hand():
    x = np.array([0, 0, 1, 0, 0.5, 0.25, 0, 0, 0, 2, 0], dtype=np.float32)
    assert D.quiet_runs_ref(x, 0.0, 1).tolist() == [[0, 2], [3, 1], [6, 3], [10, 1]]
    assert D.quiet_runs_ref(x, 0.0, 2).tolist() == [[0, 2], [6, 3]]
    assert D.quiet_runs_ref(x, 0.0, 4).tolist() == [] and D.quiet_runs_ref(x, 0.0, 4).shape == (0, 2)
    assert D.quiet_runs_ref(x, 0.25, 1).tolist() == [[0, 2], [3, 1], [5, 4], [10, 1]]          # |x| == thr is quiet
    assert D.quiet_runs_ref(x, 0.5, 3).tolist() == [[3, 6]]
    assert D.quiet_runs_ref(x, 2.0, 1).tolist() == [[0, 11]]
    y = np.array([np.nan, -0.0, 1e-40, np.inf, -np.inf, 0.0], dtype=np.float32)
    assert D.quiet_runs_ref(y, 0.0, 1).tolist() == [[1, 1], [5, 1]]                            # NaN, inf and a subnormal are loud at thr = 0
    assert D.quiet_runs_ref(y, 1e-38, 1).tolist() == [[1, 2], [5, 1]]
    assert D.quiet_runs_ref(y, np.inf, 1).tolist() == [[1, 5]]                                 # NaN stays loud
    p = np.array([-32768, 3, -3, 4, 0, 32767], dtype=np.int16)
    assert D.quiet_runs_ref(p, 3.0, 1).tolist() == [[1, 2], [4, 1]]
    assert D.quiet_runs_ref(p, 32767.0, 1).tolist() == [[1, 5]] and D.quiet_runs_ref(p, 32768.0, 1).tolist() == [[0, 6]]
    assert D.quiet_runs_ref(p, 3.5, 1).tolist() == [[1, 2], [4, 1]]


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_the_case_builders_hold_what_they_name(dtype):
    for n in D.SEAM_N:
        for name, q, min_len in D.seam_cases(n):
            assert q.shape == (n,), name
            x = D.materialize(q, dtype, n)
            assert x.dtype == dtype and np.array_equal(D.quiet_mask(x, D.THR[dtype]), q), (n, name)
    cases = dict((name, (q, m)) for name, q, m in D.seam_cases(6144))
    assert len(D.quiet_runs_ref(D.materialize(np.arange(2048) % 2 == 0, dtype), D.THR[dtype], 1)) == 1024      # 1024 runs in one chunk
    assert D.quiet_runs_ref(D.materialize(cases["whole chunks inside a run from chunk 0"][0], dtype), D.THR[dtype], 1).tolist() == [[2047, 4097]]
    got = D.quiet_runs_ref(D.materialize(cases["lengths 4, 5, 6 at min_len 5"][0], dtype), D.THR[dtype], 5)
    assert set(got[:, 1].tolist()) == {5, 6} and len(got) >= 12
    n, seam, q, q2 = D.tile_seam_case()
    assert n > D.CARRY_TILE * D.CHUNK and seam == D.CARRY_TILE * D.CHUNK
    r = D.quiet_runs_ref(D.materialize(q, dtype, 1), D.THR[dtype], 64)
    assert [seam - D.CHUNK - 1000, 2 * D.CHUNK + 1200] in r.tolist()                            # spans the tile seam, whole chunks on both sides
    assert any(s + l < seam and s + l > seam - 3 * D.CHUNK for s, l in r.tolist()) and any(seam < s < seam + 2 * D.CHUNK for s, l in r.tolist())
    assert [seam - D.CHUNK - 1000, D.CHUNK + 1000] in D.quiet_runs_ref(D.materialize(q2, dtype, 2), D.THR[dtype], 1).tolist()   # ends ON the seam


# ------------------------------------------------------------------------------------------------------------ runs_to_gaps
def _r2g(runs, n=N22, sr=22050, n_rec=N_REC, **kw):
    return G.runs_to_gaps(runs, n, sr, n_rec, **kw)


@pytest.mark.parametrize("sr,spf", [(22050, 441), (16000, 320), (44100, 882), (8000, 160), (11025, None)])
def test_a_zeroed_frame_range_gives_its_frames_back(sr, spf):
    """Frames [p, p + l) zeroed at the file's rate come back as (p, l); at 11 025 Hz a frame is 220.5 samples, so frame p starts at
    sample ceil(220.5 p) and the zeroed samples are the ones that lie wholly inside the frames."""
    n = N22 * sr // 22050
    for p, l in GAPS + [(7, 1), (51, 20)]:
        s, e = (p * spf, (p + l) * spf) if spf else (-(-p * 441 // 2), (p + l) * 441 // 2)
        assert _r2g([(s, e - s)], n, sr, merge_frames=1) == ([(p, l)], []), (sr, p, l)
        # one sample longer on either side: the cover grows by one frame on that side
        assert _r2g([(s - 1, e - s + 1)], n, sr, max_frames=21) == ([(p - 1, l + 1)], [])
        assert _r2g([(s, e - s + 1)], n, sr, max_frames=21) == ([(p, l + 1)], [])
        assert _r2g([(s - 1, e - s + 2)], n, sr, max_frames=22) == ([(p - 1, l + 2)], [])
        # one sample shorter on either side: the same frames are still touched
        if e - s > 2 * (spf or 221):
            assert _r2g([(s + 1, e - s - 2)], n, sr) == ([(p, l)], [])
    runs = [(p * spf, l * spf) if spf else (-(-p * 441 // 2), (p + l) * 441 // 2 - -(-p * 441 // 2)) for p, l in GAPS]
    assert _r2g(runs, n, sr, merge_frames=1) == (GAPS, [])
    assert _r2g(list(reversed(runs)), n, sr, merge_frames=0) == (GAPS, [])


def test_pad_frames():
    assert _r2g([(441 * 100, 441 * 5)], pad_frames=1) == ([(99, 7)], [])
    assert _r2g([(441 * 100 + 5, 10)], pad_frames=2) == ([(98, 5)], [])
    assert _r2g([(441 * 1, 441)], pad_frames=3) == ([(0, 5)], [])                               # clamped at frame 0
    assert _r2g([(441 * 296, 441)], pad_frames=3) == ([], [(293, 7, "edge")])                   # clamped at frame 300: past the usable 299
    assert _r2g([(441 * 294, 441)], pad_frames=3) == ([(291, 7)], [])
    with pytest.raises(ValueError, match="pad_frames = -1"):
        _r2g([], pad_frames=-1)


def test_merge():
    two = lambda gap: [(441 * 100, 441 * 5), (441 * (105 + gap), 441 * 4)]
    assert _r2g(two(0)) == ([(100, 9)], [])                                                     # touching
    assert _r2g(two(0), merge_frames=0) == ([(100, 9)], [])                                     # ... always
    assert _r2g(two(1)) == ([(100, 10)], [])                                                    # 1 frame apart, default merge_frames = 2
    assert _r2g(two(2)) == ([(100, 5), (107, 4)], [])                                           # exactly merge_frames apart: not merged
    assert _r2g(two(1), merge_frames=1) == ([(100, 5), (106, 4)], [])
    assert _r2g(two(5), merge_frames=6) == ([(100, 14)], []) and _r2g(two(6), merge_frames=6) == ([(100, 5), (111, 4)], [])
    # overlapping covers: two runs in one frame, and a chain of three
    assert _r2g([(441 * 50 + 10, 20), (441 * 50 + 200, 20)]) == ([(50, 1)], [])
    assert _r2g([(441 * 50, 441), (441 * 52, 441), (441 * 54, 441)]) == ([(50, 5)], [])
    assert _r2g([(441 * 50, 441), (441 * 52, 441), (441 * 54, 441)], merge_frames=1) == ([(50, 1), (52, 1), (54, 1)], [])
    # a short run inside the cover of a longer one changes nothing
    assert _r2g([(441 * 100, 441 * 5), (441 * 104 + 400, 30)]) == ([(100, 5)], [])


def test_edge_and_long():
    assert _r2g([(0, 300)]) == ([], [(0, 1, "edge")])                                           # from sample 0: leading padding
    assert _r2g([(N22 - 1000, 1000)]) == ([], [(298, 2, "edge")])                               # to sample n: trailing padding
    assert _r2g([(441 * 299, 200)]) == ([], [(299, 1, "edge")])                                 # a cover in the last frame: not usable
    assert _r2g([(441 * 298, 441)]) == ([(298, 1)], [])
    assert _r2g([(441 * 298, 441)], lim_frames=298) == ([], [(298, 1, "edge")])
    assert _r2g([(N_REC * 441 + 3, 50)]) == ([], [(300, 0, "edge")])                            # in the tail past the last whole frame
    assert _r2g([(1, 300)]) == ([(0, 1)], [])                                                   # one loud sample in front: a dropout
    assert _r2g([(441 * 100, 441 * 20)]) == ([(100, 20)], [])
    assert _r2g([(441 * 100, 441 * 20 + 1)]) == ([], [(100, 21, "long")])
    assert _r2g([(441 * 100, 441 * 12), (441 * 113, 441 * 12)]) == ([], [(100, 25, "long")])    # long after the merge
    assert _r2g([(441 * 100, 441 * 12), (441 * 113, 441 * 12)], merge_frames=1) == ([(100, 12), (113, 12)], [])
    assert _r2g([(441 * 100, 441 * 12)], max_frames=11) == ([], [(100, 12, "long")])
    got = _r2g([(0, 300), (441 * 2, 441 * 3), (441 * 100, 441 * 30), (N22 - 1000, 1000)])
    assert got == ([(2, 3)], [(0, 1, "edge"), (100, 30, "long"), (298, 2, "edge")])
    with pytest.raises(ValueError, match=r"run 0 = samples \[5, 5\)"):
        _r2g([(5, 0)])
    with pytest.raises(ValueError, match=r"is not a run of a recording of 100 samples"):
        _r2g([(90, 11)], n=100)


def test_the_gaps_pass_the_planner_unchanged():
    """On the geometry of tests/test_gpu_long.py (300 frames, clips of 75, context 15): the detected gaps of the zeroed GAPS are what
    normalize_gaps returns for them and plan_contexts plans them as it plans GAPS; at the default merge_frames the two gaps one
    frame apart are one."""
    runs = D.quiet_runs_ref(D.mask_of(N22, [(441 * p, 441 * (p + l)) for p, l in GAPS]).astype(np.float32) - 1, 0.0, 110)
    gaps, skipped = _r2g(runs.tolist(), merge_frames=1, lim_frames=N_REC - CLIP + LIM)
    assert gaps == GAPS and skipped == []
    assert G.normalize_gaps([gaps], [N_REC]) == [gaps]
    kw = dict(clip_frames=CLIP, min_context=CTX, lim_frames=LIM)
    assert G.plan_contexts(gaps, N_REC, **kw) == G.plan_contexts(GAPS, N_REC, **kw)
    merged, _ = _r2g(runs.tolist())
    assert merged == [(2, 3), (100, 10), (140, 6), (292, 5)] and len(G.plan_contexts(merged, N_REC, **kw)) == 4
    # random runs: whatever comes out is sorted, disjoint, at least merge_frames apart, and plannable
    rng = np.random.default_rng(3)
    for trial in range(20):
        q = D.random_mask(N22, 0.004, trial) & D.random_mask(N22, 0.001, 100 + trial)
        gaps, skipped = _r2g(D.quiet_runs_ref(q.astype(np.float32) - 1, 0.0, int(rng.integers(1, 200))).tolist(), lim_frames=N_REC - CLIP + LIM)
        assert gaps == sorted(gaps) and all(b[0] - (a[0] + a[1]) >= 2 for a, b in zip(gaps, gaps[1:]))
        assert all(0 < l <= 20 and p + l <= N_REC - 1 for p, l in gaps) and all(why in ("edge", "long") for _, _, why in skipped)
        try:
            G.plan_contexts(gaps, N_REC, **kw)
        except ValueError as e:                                       # only the per-context span limit may refuse a crowded recording
            assert "more than the 16" in str(e), e


# ------------------------------------------------------------------------------------------------------------ predict.yaml
def _yaml(tmp_path, extra, drop=("mask",)):
    data = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "iea_predict.yaml")))
    for key in drop:
        data.pop(key, None)
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_detect_key(tmp_path):
    defaults = {"threshold": 0.0, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0}
    assert load_predict_config(_yaml(tmp_path, "long: {}\n")).detect is None
    assert load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {}\n")).detect == defaults
    assert load_predict_config(_yaml(tmp_path, "long: {}\ndetect:\n")).detect == defaults
    cfg = load_predict_config(_yaml(tmp_path, "long:\n  clip_s: 1.5\n  context_s: 0.3\ndetect:\n  threshold: 0.001\n  min_ms: 2\n  max_ms: 200\n  pad_frames: 1\n"))
    assert cfg.detect == {"threshold": 0.001, "min_ms": 2.0, "max_ms": 200.0, "pad_frames": 1} and cfg.long["clip_s"] == 1.5 and cfg.masks is None
    with pytest.raises(ValueError, match="unknown key `thresh` in `detect:`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect:\n  thresh: 0\n"))
    for key in defaults:
        with pytest.raises(ValueError, match=f"detect.{key} = -1(.0)? is negative"):
            load_predict_config(_yaml(tmp_path, f"long: {{}}\ndetect:\n  {key}: -1\n"))
    with pytest.raises(ValueError, match="`detect:` must be a mapping"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: 4\n"))
    with pytest.raises(ValueError, match="`detect:` must be a mapping"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: [1, 2]\n"))
    with pytest.raises(ValueError, match="`detect:` needs a `long:` mapping"):
        load_predict_config(_yaml(tmp_path, "detect: {}\n"))
    with pytest.raises(ValueError, match="either `detect:` .* or `mask:` / `masks:`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {}\nmasks:\n  - {start_pos_in_sec: 1.0, end_pos_in_sec: 1.1}\n"))
    with pytest.raises(ValueError, match="either `detect:` .* or `mask:` / `masks:`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {}\n", drop=()))
    # the messages of `long:` are what they were
    with pytest.raises(ValueError, match="unknown key `clip_frames` in `long:`"):
        load_predict_config(_yaml(tmp_path, "long:\n  clip_frames: 200\ndetect: {}\n"))


# ------------------------------------------------------------------------------------------------------------ ABI
def test_the_abi_declares_the_call():
    from speech_inpainting_amd import native
    header = open(os.path.join(ROOT, "include", "si_hip.h")).read()
    flat = " ".join(header.split())
    assert ("int si_quiet_runs(si_ctx* ctx, const void* x, int is_pcm16, int n, float threshold, int min_len, int32_t* runs, int max_runs, "
            "int32_t* n_runs, si_stream_t stream);") in flat
    assert "si_quiet_runs" in native.EXPORTS and hasattr(native.NativeContext, "quiet_runs")
    assert "I_ea/predict.py:85-90" in header[header.index("si_quiet_runs"):]
    assert "detect_kernels.hip" in open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "Makefile")).read()
