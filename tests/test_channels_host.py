"""Interleaved multi-channel files, the parts that need no GPU: the three declarations and their bindings, the
`detect: {channels: ...}` key of predict.yaml, the host planning of a two-channel gap set written out by hand, and the joint-detection
reference on a 12-sample example."""
import os
import re

import numpy as np
import pytest
import yaml

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from speech_inpainting_amd.config import load_predict_config
from tests import channels_ref as CH
from tests import detect_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("si_quiet_runs_ch", "si_cut_rate_ch", "si_patch_rate_ch")


# ------------------------------------------------------------------------------------------------------------ ABI
def _declaration(hdr, name):
    m = re.search(r"^int " + name + r"\((.*?)\);", hdr, re.S | re.M)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_the_three_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "si_hip.h")).read()
    assert re.search(r"#define SI_ABI_VERSION 3\b", hdr)
    assert int(re.search(r"#define SI_MAX_CHANNELS (\d+)\b", hdr).group(1)) == native.SI_MAX_CHANNELS == G.MAX_CHANNELS == 8

    lib = native.load_library() if os.path.exists(native.LIB_PATH) else None
    assert lib is None or lib.si_version() == 3
    for name in NEW:
        assert name in native.EXPORTS
        args = _declaration(hdr, name)
        mono = _declaration(hdr, name[:-3])
        assert len(args) == len(mono) + 2 and (lib is None or len(getattr(lib, name).argtypes) == len(args)), name
        assert [a for a in args if a not in ("int channels", "int channel")] == mono, name     # the mono signature + the two, nothing else
        assert args[0] == "si_ctx* ctx" and args[-1] == "si_stream_t stream"
    assert _declaration(hdr, "si_quiet_runs_ch")[4:6] == ["int channels", "int channel"]
    assert _declaration(hdr, "si_cut_rate_ch")[4:6] == ["int channels", "int channel"]
    assert _declaration(hdr, "si_patch_rate_ch")[4:6] == ["int channels", "int channel"]
    api = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "api.hip")).read()
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", api, re.M), name


# ------------------------------------------------------------------------------------------------------------ predict.yaml
def _yaml(tmp_path, extra, drop=("mask",)):
    data = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "iea_predict.yaml")))
    for key in drop:
        data.pop(key, None)
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_detect_channels_key(tmp_path):
    defaults = {"threshold": 0.0, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0}
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file}\ndetect: {}\n"))
    assert cfg.detect == defaults and cfg.detect_channels == "each"
    assert load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {}\n")).detect_channels == "each"          # the key absent: nothing is refused
    for mode in ("each", "joint"):
        cfg = load_predict_config(_yaml(tmp_path, f"long: {{rate: file, feed: contexts}}\ndetect: {{channels: {mode}, min_ms: 2}}\n"))
        assert cfg.detect_channels == mode and cfg.detect == {**defaults, "min_ms": 2.0} and cfg.long_feed == "contexts"
    with pytest.raises(ValueError, match="detect.channels = 'both': each .* or joint"):
        load_predict_config(_yaml(tmp_path, "long: {rate: file}\ndetect: {channels: both}\n"))
    with pytest.raises(ValueError, match=r"detect.channels needs `long: \{rate: file\}`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {channels: joint}\n"))
    with pytest.raises(ValueError, match=r"detect.channels needs `long: \{rate: file\}`"):
        load_predict_config(_yaml(tmp_path, "long: {rate: 22050}\ndetect: {channels: each}\n"))
    with pytest.raises(ValueError, match="unknown key `channel` in `detect:` .*channels"):
        load_predict_config(_yaml(tmp_path, "long: {rate: file}\ndetect: {channel: each}\n"))


# ------------------------------------------------------------------------------------------------------------ planning
def test_two_channel_plan_by_hand():
    """1000 frames, clips of 200 with 50 of context.  Channel 0: gaps at 100 (5 frames) and 130 (4) share a context, 600 (6) has its own.
    Channel 1: one gap at 400 (3), given out of order with nothing else.  Contexts in (channel, start) order, gap indices and label
    offsets in (channel, gap) order."""
    per = [[(600, 6), (100, 5), (130, 4)], [(400, 3)]]
    ctxs, off = G.plan_channel_contexts(per, 1000, 200, 50)
    assert off == [0, 3, 4]
    assert [(k["channel"], k["start"], k["own_index"]) for k in ctxs] == [(0, 17, [0, 1]), (0, 503, [2]), (1, 301, [3])]
    assert ctxs[0]["own"] == [(83, 5), (113, 4)] and ctxs[1]["own"] == [(97, 6)] and ctxs[2]["own"] == [(99, 3)]
    assert all(k["foreign"] == [] and k["frames"] == 200 for k in ctxs)
    assert G.gap_label_off(ctxs, off[-1]) == [0, 5, 9, 15, 18]
    # every channel's contexts are plan_contexts' on that channel alone
    for c, g in enumerate(per):
        alone = G.plan_contexts(g, 1000, 200, 50)
        mine = [k for k in ctxs if k["channel"] == c]
        assert [(k["start"], k["own"], k["foreign"]) for k in mine] == [(k["start"], k["own"], k["foreign"]) for k in alone]
        assert [[i - off[c] for i in k["own_index"]] for k in mine] == [k["own_index"] for k in alone]
    # passes of two contexts: the boundary falls inside channel 0, and the second pass holds both channels
    assert G.pass_channels(ctxs[0:2]) == [(0, 0, 2)] and G.pass_channels(ctxs[2:4]) == [(1, 0, 1)]
    assert G.pass_channels(ctxs[1:3]) == [(0, 0, 1), (1, 1, 2)] and G.pass_channels(ctxs) == [(0, 0, 2), (1, 2, 3)] and G.pass_channels([]) == []
    # a channel without gaps has no context and an empty index range
    ctxs, off = G.plan_channel_contexts([[], [(400, 3)], []], 1000, 200, 50)
    assert off == [0, 0, 1, 1] and [(k["channel"], k["own_index"]) for k in ctxs] == [(1, [0])] and G.gap_label_off(ctxs, 1) == [0, 3]
    assert G.plan_channel_contexts([[], []], 1000, 200, 50) == ([], [0, 0, 0])
    with pytest.raises(ValueError, match=r"channel 1: recording: gap 1 = frames \[402, 404\) overlaps gap 0"):
        G.plan_channel_contexts([[(10, 3)], [(400, 3), (402, 2)]], 1000, 200, 50)


def test_gaps_or_channel_gaps():
    assert G.channel_gap_lists([(1, 2)], None, 3) == [[(1, 2)]] * 3
    assert G.channel_gap_lists(None, ([(1, 2)], ()), 2) == [[(1, 2)], []]
    with pytest.raises(ValueError, match="both gaps and channel_gaps"):
        G.channel_gap_lists([(1, 2)], [[(1, 2)], []], 2)
    with pytest.raises(ValueError, match="both gaps and channel_gaps"):
        G.channel_gap_lists([], [[], []], 2)
    with pytest.raises(ValueError, match="neither gaps nor channel_gaps"):
        G.channel_gap_lists(None, None, 2)
    with pytest.raises(ValueError, match="3 lists for a file of 2 channels"):
        G.channel_gap_lists(None, [[], [], []], 2)


# ------------------------------------------------------------------------------------------------------------ the joint reference
def test_the_joint_reference_on_twelve_samples():
    #             0     1    2    3     4    5    6    7       8    9    10   11
    a = np.array([0.0, 0.0, 0.5, 0.0, -0.0, 0.0, 0.0, np.nan, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)
    b = np.array([0.0, 0.3, 0.0, 0.0, 0.0, 0.0, -0.1, 0.0, 0.0, 0.0, 0.0, 0.7], dtype=np.float32)
    x = np.stack([a, b], axis=1)
    assert CH.joint_signal(x, 0.0).tolist() == [0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1]
    assert CH.joint_runs_ref(x, 0.0, 1).tolist() == [[0, 1], [3, 3], [8, 3]]
    assert CH.joint_runs_ref(x, 0.0, 2).tolist() == [[3, 3], [8, 3]]
    assert CH.joint_runs_ref(x, 0.1, 1).tolist() == [[0, 1], [3, 4], [8, 3]]                    # |-0.1| = thr is quiet; NaN stays loud
    assert D.quiet_runs_ref(a, 0.0, 1).tolist() == [[0, 2], [3, 4], [8, 4]] and D.quiet_runs_ref(b, 0.0, 1).tolist() == [[0, 1], [2, 4], [7, 4]]
    # one channel: the joint answer is the channel's own
    assert CH.joint_runs_ref(a[:, None], 0.0, 1).tolist() == D.quiet_runs_ref(a, 0.0, 1).tolist()
    p = np.array([[-32768, 0], [0, 0], [3, -3], [4, 0]], dtype=np.int16)
    assert CH.joint_runs_ref(p, 3.0, 1).tolist() == [[1, 2]] and CH.joint_runs_ref(p, 32768.0, 1).tolist() == [[0, 4]]
