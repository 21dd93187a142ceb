"""Dropouts by windowed RMS level, the parts that need no GPU: the declaration and its binding, the `win_ms:` key of
`detect:` in predict.yaml with its refusals and the new config field, the routing of kind="level" through find_gaps, conceal_recording
and conceal_file, the win_ms -> half rounding with its limit, and the int16 scaling on the way from predict.yaml to the engine."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import yaml

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from speech_inpainting_amd import predict as P
from speech_inpainting_amd.config import load_predict_config
from speech_inpainting_amd.engine import InpaintingEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ ABI
def test_the_entry_point_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "si_hip.h")).read()
    assert re.search(r"#define SI_ABI_VERSION 3\b", hdr)
    m = re.search(r"^int si_level_runs\((.*?)\);", hdr, re.S | re.M)
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["si_ctx* ctx", "const void* x", "int is_pcm16", "int n", "int channels", "int channel", "int half", "float threshold",
                    "float rel_threshold", "int min_len", "int32_t* runs", "int max_runs", "int32_t* n_runs", "float* threshold_out",
                    "si_stream_t stream"]
    dead = re.search(r"^int si_dead_runs\((.*?)\);", hdr, re.S | re.M).group(1).replace("\n", " ")
    assert [a for a in args if a != "int half"] == [a.strip() for a in dead.split(",") if a.strip() not in ("int kind", "float held_tol")]
    assert int(re.search(r"#define SI_LEVEL_MAX_HALF (\d+)\b", hdr).group(1)) == native.LEVEL_MAX_HALF == G.LEVEL_MAX_HALF == 1024
    doc = hdr[hdr.index("Dropouts by windowed RMS level"):m.start()]
    for phrase in ("The reference has no detection", "I_ea/predict.py:85-90", "max(threshold, fl32(rel_threshold * peak))", "BY ADDITIONS ONLY",
                   "no window is a difference of running sums", "cnt * 2^-52 * E", "fl64(((double)T * (double)T) * cnt(i))", "UNION of the low windows",
                   "never the adjacent elements", "EVERY channel's dead_c holds", "half = 0", "exactly p + 1", "half outside 0 ..", "not finite",
                   "no atomics"):
        assert phrase in doc, phrase
    assert re.search(r"si_level_runs\s+<- nothing the reference computes", hdr)
    assert "si_level_runs" in native.EXPORTS and len(set(native.EXPORTS)) == len(native.EXPORTS)
    assert callable(native.NativeContext.level_runs) and callable(InpaintingEngine.find_level_runs)
    api = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "api.hip")).read()
    assert re.search(r"^int si_level_runs\(", api, re.M)
    kern = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "detect_kernels.hip")).read()
    assert "detect_level_kernel" in kern and '"detect_level"' not in kern       # profiled as "detect_dead": tests/poison.py's family lists are closed
    if os.path.exists(native.LIB_PATH):
        lib = native.load_library()
        assert lib.si_version() == 3 and len(lib.si_level_runs.argtypes) == len(args) == 15


# ------------------------------------------------------------------------------------------------------------ predict.yaml
def _yaml(tmp_path, extra, drop=("mask",)):
    data = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "iea_predict.yaml")))
    for key in drop:
        data.pop(key, None)
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_win_ms(tmp_path):
    defaults = {"threshold": 0.0, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0}
    assert load_predict_config(_yaml(tmp_path, "long: {}\n")).detect_level is None
    cfg = load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {}\n"))
    assert cfg.detect == defaults and cfg.detect_dead == {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0} and cfg.detect_level == {"win_ms": 2.0}
    cfg = load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: level, threshold: 0.0005}\n"))
    assert cfg.detect == {**defaults, "threshold": 0.0005} and cfg.detect_dead == {"kind": "level", "rel_threshold": 0.0, "held_tol": 0.0}
    assert cfg.detect_level == {"win_ms": 2.0}
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file}\ndetect: {kind: level, win_ms: 3.5, rel_threshold: 0.001, channels: joint}\n"))
    assert cfg.detect == defaults and cfg.detect_level == {"win_ms": 3.5} and cfg.detect_dead["rel_threshold"] == 0.001 and cfg.detect_channels == "joint"
    assert load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: level, win_ms: 0}\n")).detect_level == {"win_ms": 0.0}
    with pytest.raises(ValueError, match="detect.win_ms needs `kind: level`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {win_ms: 2}\n"))
    with pytest.raises(ValueError, match="detect.win_ms needs `kind: level` .kind: held"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: held, win_ms: 2}\n"))
    for bad in ("-1", ".nan", ".inf"):
        with pytest.raises(ValueError, match="detect.win_ms = .* is negative or not finite"):
            load_predict_config(_yaml(tmp_path, f"long: {{}}\ndetect: {{kind: level, win_ms: {bad}}}\n"))
    with pytest.raises(ValueError, match="detect.held_tol = 0.001 with `kind: level`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: level, held_tol: 0.001}\n"))
    # the two messages of before keep their words, the new kind and key come after them
    with pytest.raises(ValueError, match=r"detect.kind = 'rms': quiet .* held .* or any, or level \(the RMS level of a window of win_ms"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: rms}\n"))
    with pytest.raises(ValueError, match=r"unknown key `win` in `detect:` \(it takes threshold, min_ms, max_ms, pad_frames, channels, kind, rel_threshold, held_tol\) and, with kind: level, win_ms"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: level, win: 2}\n"))


# ------------------------------------------------------------------------------------------------------------ win_ms -> half
def test_win_ms_to_half_and_its_limit():
    assert [G.level_half(2.0, sr) for sr in (8000, 22050, 48000, 192000)] == [8, 22, 48, 192]
    assert G.level_half(0.0, 48000) == 0 and G.level_half(1.0, 22050) == 11 and G.level_half(5.0, 44100) == 110
    assert G.level_half(0.1, 8000) == 0 and G.level_half(0.2, 8000) == 1 and G.level_half(3.0, 22050) == 33        # 0.4 | 0.8 | 33.075
    # the largest window per rate: half = 1024 is served, the next sample is refused with the limit in milliseconds
    for sr, most in ((8000, 256.0), (22050, 92.879), (48000, 42.666), (192000, 10.666)):
        assert G.level_half(most, sr) == 1024, sr
        assert G.level_half(2000.0 * 1024 / sr, sr) == 1024
        with pytest.raises(ValueError, match=rf"at {sr} Hz is a half window of more than 1024 samples: at most win_ms = {most} at this rate"):
            G.level_half(2000.0 * 1025 / sr, sr)
    with pytest.raises(ValueError, match="more than 1024 samples"):
        G.level_half(float("inf"), 48000)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="not negative"):
            G.level_half(bad, 48000)


# ------------------------------------------------------------------------------------------------------------ routing
class _Recorder:
    """Stands in for an engine under find_gaps: records which detector was called and with what."""
    DEAD_KINDS = InpaintingEngine.DEAD_KINDS

    def __init__(self):
        self.calls = []

    def find_quiet_runs(self, *a, **kw):
        self.calls.append(("quiet", a[1:], kw))
        return torch.tensor([[441 * 10, 441 * 3]], dtype=torch.int32)

    def find_dead_runs(self, *a, **kw):
        self.calls.append(("dead", a[1:], kw))
        return torch.tensor([[441 * 10, 441 * 3]], dtype=torch.int32), 0.125

    def find_level_runs(self, *a, **kw):
        self.calls.append(("level", a[1:], kw))
        return torch.tensor([[441 * 10, 441 * 3]], dtype=torch.int32), 0.25


def test_find_gaps_routes_kind_level_and_nothing_else_to_the_level_detector():
    x = torch.zeros(22050)
    rec = _Recorder()
    out = InpaintingEngine.find_gaps(rec, x, threshold=0.01, min_ms=5.0, kind="level")
    want = dict(half=22, threshold=0.01, rel_threshold=0.0, min_len=110, channel=None, return_threshold=True)
    assert rec.calls == [("level", (), want)]
    assert sorted(out) == ["gaps", "runs", "skipped", "threshold"] and out["gaps"] == [(10, 3)] and out["threshold"] == 0.25
    rec.calls.clear()
    InpaintingEngine.find_gaps(rec, x.reshape(-1, 2), 48000, 0.5, kind="level", rel_threshold=1e-3, win_ms=3.0, channel=-1)
    assert rec.calls == [("level", (), dict(half=72, threshold=0.5, rel_threshold=1e-3, min_len=240, channel=-1, return_threshold=True))]
    with pytest.raises(ValueError, match="held_tol = 0.5 with kind = 'level'"):
        InpaintingEngine.find_gaps(rec, x, kind="level", held_tol=0.5)
    with pytest.raises(ValueError, match="at most win_ms = 92.879 at this rate"):
        InpaintingEngine.find_gaps(rec, x, kind="level", win_ms=100.0)
    # every other kind is called as it was, whatever win_ms says
    rec.calls.clear()
    InpaintingEngine.find_gaps(rec, x, threshold=0.01, win_ms=7.0)
    InpaintingEngine.find_gaps(rec, x, threshold=0.01, kind="held", win_ms=7.0)
    assert rec.calls == [("quiet", (0.01, 110), {"channel": None}),
                         ("dead", ("held", 0.01, 0.0, 0.0, 110), {"channel": None, "return_threshold": True})]


def test_conceal_routes_pass_win_ms_with_kind_level_alone():
    calls = []

    def find_gaps(*a, **kw):
        calls.append(kw)
        return {"gaps": [], "skipped": [], "runs": None, "threshold": 0.5}

    patched = lambda *a, **kw: {"patched": torch.zeros(4)}
    eng = types.SimpleNamespace(device=torch.device("cpu"), recording_frames=lambda *a: (100, 100), find_gaps=find_gaps, patch_file=patched,
                                patch_recording=patched)
    x = torch.zeros(48000)
    out = InpaintingEngine.conceal_file(eng, x, 48000, 0.25, kind="level", win_ms=3.0)
    assert calls[-1] == {"channel": None, "kind": "level", "rel_threshold": 0.0, "held_tol": 0.0, "win_ms": 3.0} and out["threshold"] == 0.5
    InpaintingEngine.conceal_file(eng, x, 48000, 0.25, kind="level")
    assert calls[-1]["win_ms"] == 2.0
    InpaintingEngine.conceal_file(eng, x.reshape(-1, 2), 48000, 0.25, kind="level", detect="each")
    assert [c["channel"] for c in calls[-2:]] == [0, 1] and all(c["win_ms"] == 2.0 for c in calls[-2:])
    InpaintingEngine.conceal_file(eng, x, 48000, 0.25, kind="any", win_ms=3.0)
    assert calls[-1] == {"channel": None, "kind": "any", "rel_threshold": 0.0, "held_tol": 0.0}         # the call of before
    InpaintingEngine.conceal_recording(eng, x[:22050], kind="level", win_ms=1.0, rel_threshold=0.1)
    assert calls[-1] == {"kind": "level", "rel_threshold": 0.1, "held_tol": 0.0, "win_ms": 1.0}
    InpaintingEngine.conceal_recording(eng, x[:22050], win_ms=1.0)
    assert calls[-1] == {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0}


def test_find_level_runs_checks_its_window_before_the_device():
    eng = types.SimpleNamespace()
    for kw, msg in ((dict(), "win = its odd length"), (dict(win=5, half=2), "not both"), (dict(win=4), "win = 4: an odd number"), (dict(win=0), "win = 0"),
                    (dict(half=-1), "half = -1 samples, outside 0 .. 1024"), (dict(half=1025), "half = 1025 samples"), (dict(win=2051), "half = 1025"),
                    (dict(half=1.5), "half = 1.5")):
        with pytest.raises(ValueError, match=msg):
            InpaintingEngine.find_level_runs(eng, np.zeros(8, np.float32), **kw)


# ------------------------------------------------------------------------------------------------------------ int16 scaling
def test_the_threshold_is_scaled_for_an_int16_file_and_win_ms_is_not(tmp_path, capsys):
    level = types.SimpleNamespace(detect_dead={"kind": "level", "rel_threshold": 1e-3, "held_tol": 0.0}, detect_level={"win_ms": 3.0})
    assert P.level_keywords(level) == {"win_ms": 3.0}
    assert P.level_keywords(types.SimpleNamespace(detect_dead={"kind": "any", "rel_threshold": 0.0, "held_tol": 0.0}, detect_level={"win_ms": 3.0})) == {}
    assert P.level_keywords(types.SimpleNamespace(detect_dead=None)) == {}
    assert P.level_keywords(types.SimpleNamespace(detect_dead={"kind": "level", "rel_threshold": 0.0, "held_tol": 0.0})) == {"win_ms": 2.0}
    from scipy.io import wavfile
    calls = []

    def find_gaps(x, sr, thr, *a, **kw):
        calls.append((x.dtype, thr, kw))
        return {"gaps": [(10, 3)], "skipped": [], "runs": None, "threshold": thr}

    engine = types.SimpleNamespace(recording_frames=lambda n22, clip: (100, 100), find_gaps=find_gaps)
    pcm = (np.arange(22050) % 200 - 100).astype(np.int16)
    for name, data, T, unit in (("pcm.wav", pcm, 16.0, "int16 steps"), ("f32.wav", (pcm / 32768.0).astype(np.float32), 16.0 / 32768, "full scale")):
        wavfile.write(tmp_path / name, 22050, data)
        cfg = types.SimpleNamespace(wave_path=str(tmp_path / name), detect={"threshold": 16.0 / 32768, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0},
                                    detect_dead=level.detect_dead, detect_level=level.detect_level)
        assert P._detect_gaps(cfg, engine, data.astype(np.float32), 22050, 22050, 110, 200, 50, str(tmp_path)) == [(10, 3)]
        assert json.loads((tmp_path / "gaps.json").read_text()) == {"gaps": [[10, 3]], "skipped": [], "kind": "level", "T": T, "win_ms": 3.0}
        assert f"Detection kind = level, effective threshold T = {T} ({unit}), window win_ms = 3.0" in capsys.readouterr().out
    assert calls[0] == (np.int16, 16.0, {"kind": "level", "rel_threshold": 1e-3, "held_tol": 0.0, "win_ms": 3.0})
    assert calls[1] == (np.float32, 16.0 / 32768, {"kind": "level", "rel_threshold": 1e-3, "held_tol": 0.0, "win_ms": 3.0})
