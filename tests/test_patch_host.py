"""Patch mode, host side: the cross-fade ramp, the blend regions, the generator windows that hold them, and the
`patch:` key of predict.yaml.  Pure Python, no GPU."""
import os

import numpy as np
import pytest

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd.config import load_predict_config

HOP, RF, T_OUT = 256, 16, 129                      # the V1 generator's hop and receptive radius in frames; a 1.5 s clip's stretched frames
N22, N_OUT = 33075, 33024


@pytest.mark.parametrize("fade", [1, 2, 110, 300, 441])
def test_fade_ramp_is_the_float64_formula_rounded_once(fade):
    r = G.fade_ramp(fade)
    assert r.dtype == np.float32 and r.shape == (fade,)
    i = np.arange(fade, dtype=np.float64)
    ref = 0.5 * (1.0 - np.cos(np.pi * (i + 0.5) / fade))
    assert np.array_equal(r, ref.astype(np.float32))
    assert np.all(r > 0) and np.all(r < 1) and np.all(np.diff(r) > 0)
    # ramp[i] + ramp[fade - 1 - i] = 1 in exact arithmetic: each term is within half an ulp, of a value <= 1, of its float64 value
    assert np.max(np.abs(r.astype(np.float64) + r[::-1].astype(np.float64) - 1.0)) <= 2.0 ** -24


def test_fade_zero_is_a_hard_splice_and_negative_is_refused():
    assert G.fade_ramp(0).shape == (0,) and G.fade_ramp(0).dtype == np.float32
    with pytest.raises(ValueError, match="negative"):
        G.fade_ramp(-1)
    w = G.blend_weights([(1000, 500)], N22, N_OUT, 0)
    assert np.array_equal(np.flatnonzero(w), np.arange(1000, 1500)) and np.all(w[1000:1500] == 1)


def test_blend_regions_clamp_at_both_ends_and_skip_empty_and_late_spans():
    spans = [(0, 1323), (5000, 0), (32800, 200), (33024, 51), (33060, 10)]
    regs = G.blend_regions(spans, N22, N_OUT, 110)
    assert regs[0] == (0, 1433)                                  # clamped at sample 0
    assert regs[1] is None                                       # no samples
    assert regs[2] == (32690, N_OUT)                             # e + fade = 33110 clamped at lim = min(n22, n_out)
    assert regs[3] is None and regs[4] is None                   # start at / beyond the generated samples
    assert G.blend_regions([(100, 50)], 120, 4096, 10) == [(90, 120)]      # lim is the clip's own length when that is the smaller
    w = G.blend_weights(spans, N22, N_OUT, 110)
    assert w.shape == (N22,) and np.all(w[N_OUT:] == 0) and np.all(w[1433:32690] == 0)
    assert np.all(w[:1323] == 1) and np.all(w[32800:33000] == 1)
    ramp = G.fade_ramp(110)
    assert np.array_equal(w[1323:1433], ramp[::-1]) and np.array_equal(w[32690:32800], ramp)
    assert np.array_equal(w[33000:N_OUT], ramp[::-1][:24])       # the fall, cut at lim


def test_blend_weights_take_the_maximum_where_ramps_overlap():
    # gaps (30, 4) and (35, 4) of the GPU test: spans [13230, 14994) and [15435, 17199), 441 samples apart, fade 300
    spans = G.spans22([[(30, 4), (35, 4)]], [N22])[0]
    assert spans == [(13230, 1764), (15435, 1764)]
    w = G.blend_weights(spans, N22, N_OUT, 300)
    ramp = G.fade_ramp(300)
    m = np.arange(14994, 15435)
    fall = np.where(m - 14994 < 300, ramp[np.clip(299 - (m - 14994), 0, 299)], 0)
    rise = np.where(m >= 15435 - 300, ramp[np.clip(m - (15435 - 300), 0, 299)], 0)
    assert np.array_equal(w[14994:15435], np.maximum(fall, rise).astype(np.float32))
    assert np.all(w[14994:15435] > 0)


def _inside_kept(regs, wins, which):
    for r, k in zip(regs, which):
        if r is None:
            assert k == -1
            continue
        k0, k1 = G.kept_region(*wins[k], T_OUT, RF)
        assert k0 * HOP <= r[0] and r[1] <= k1 * HOP


@pytest.mark.parametrize("fade", [0, 110, 300])
@pytest.mark.parametrize("gaps,n_win", [([(30, 4), (35, 4)], 1), ([(5, 3), (60, 10)], 2), ([(20, 5)], 1), ([(0, 3), (60, 10)], 2), ([], 0)])
def test_plan_patch_windows_counts_and_keeps_every_region(gaps, n_win, fade):
    spans = G.spans22([gaps], [N22])[0]
    regs = G.blend_regions(spans, N22, N_OUT, fade)
    wins, which = G.plan_patch_windows(regs, T_OUT, HOP, RF)
    assert len(wins) == n_win and len(which) == len(gaps)
    assert all(0 <= a < b <= T_OUT for a, b in wins) and all(wins[i][1] < wins[i + 1][0] for i in range(len(wins) - 1))
    _inside_kept(regs, wins, which)
    if gaps:
        assert sum(b - a for a, b in wins) < T_OUT               # a fraction of the clip


def test_plan_patch_windows_merges_touching_windows_and_keeps_clip_edges():
    # regions whose windows exactly touch: frames [20, 21) + rf -> [4, 37), frames [53, 54) - rf -> [37, 70)
    wins, which = G.plan_patch_windows([(20 * HOP, 21 * HOP), (53 * HOP, 54 * HOP)], T_OUT, HOP, RF)
    assert wins == [(4, 70)] and which == [0, 0]
    wins, which = G.plan_patch_windows([(20 * HOP, 21 * HOP), (54 * HOP, 55 * HOP)], T_OUT, HOP, RF)
    assert wins == [(4, 37), (38, 71)] and which == [0, 1]
    # a gap at frame 0 and one ending at the last frame: clip-edge windows, whose kept region reaches the real edge
    regs = [(0, 300), (N_OUT - 300, N_OUT)]
    wins, which = G.plan_patch_windows(regs, T_OUT, HOP, RF)
    assert wins[0][0] == 0 and wins[-1][1] == T_OUT
    assert G.kept_region(*wins[0], T_OUT, RF)[0] == 0 and G.kept_region(*wins[-1], T_OUT, RF)[1] == T_OUT
    _inside_kept(regs, wins, which)
    # regions in any order, None entries skipped
    wins2, which2 = G.plan_patch_windows([regs[1], None, regs[0]], T_OUT, HOP, RF)
    assert wins2 == wins and which2 == [len(wins) - 1, -1, 0]


def _yaml(tmp_path, extra):
    src = open(os.path.join(os.path.dirname(__file__), "golden", "iea_predict.yaml")).read()
    p = tmp_path / "predict.yaml"
    p.write_text(src + "\n" + extra)
    return str(p)


def test_predict_yaml_patch_key(tmp_path):
    assert load_predict_config(_yaml(tmp_path, "")).patch_fade is None
    cfg = load_predict_config(_yaml(tmp_path, "patch:\n  fade_ms: 5\n"))
    assert cfg.patch_fade_ms == 5.0 and cfg.patch_fade == 110
    assert load_predict_config(_yaml(tmp_path, "patch: {}\n")).patch_fade == 110          # the default: 5 ms
    assert load_predict_config(_yaml(tmp_path, "patch:\n  fade_ms: 0\n")).patch_fade == 0
    with pytest.raises(ValueError, match="fade_samples"):
        load_predict_config(_yaml(tmp_path, "patch:\n  fade_samples: 3\n"))
    with pytest.raises(ValueError, match="mapping"):
        load_predict_config(_yaml(tmp_path, "patch: 5\n"))
