"""Corrupted blocks by second-difference level, the parts that need no GPU: the declaration and its binding, `kind:
burst` in predict.yaml with its refusals, the routing of kind="burst" through find_gaps, conceal_recording and conceal_file -- and of
every other kind as before --, the T = 0 refusal, the [0, 4] range of rel_threshold, and the PCM scaling on the way from predict.yaml to
the engine."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import yaml

from speech_inpainting_amd import native
from speech_inpainting_amd import predict as P
from speech_inpainting_amd.config import load_predict_config
from speech_inpainting_amd.engine import InpaintingEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ ABI
def test_the_entry_point_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "si_hip.h")).read()
    assert re.search(r"#define SI_ABI_VERSION 3\b", hdr)
    m = re.search(r"^int si_burst_runs\((.*?)\);", hdr, re.S | re.M)
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    level = re.search(r"^int si_level_runs\((.*?)\);", hdr, re.S | re.M).group(1).replace("\n", " ")
    assert args == [a.strip() for a in level.split(",")] and len(args) == 15              # si_level_runs' argument list
    doc = hdr[hdr.index("Corrupted blocks by second-difference level"):m.start()]
    for phrase in ("The reference has no detection", "I_ea/predict.py:85-90", "max(threshold, fl32(rel_threshold * peak))", "1 <= k <= n - 2 ONLY",
                   "x[k - 1] - 2 x[k] + x[k + 1] in int32", "131 070", "< 2^26", "24-bit steps",
                   "fl64(fl64((double)x[k - 1] + (double)x[k + 1]) - 2 * (double)x[k])", "fl64(D * D)", "two roundings and one", "NO contraction",
                   "any of x[k - 1], x[k], x[k + 1] is NaN or +-inf", "[max(1, i - h), min(n - 2, i + h)]", "which may be 0", "BY ADDITIONS ONLY",
                   "cnt * 2^-52 * E", "cnt(i) >= 1", "E(i) >= lim(i) = fl64(((double)T * (double)T) * cnt(i))", "union of the hot windows",
                   "never the adjacent elements", "every channel's dead_c holds", "half = 0, hot(i) <=> |d(i)| >= T", "n < 3 gives zero runs",
                   "never hot", "[0, 4]", "no atomics"):
        assert phrase in doc, phrase
    assert re.search(r"si_burst_runs\s+<- nothing the reference computes", hdr)
    assert "si_burst_runs" in native.EXPORTS and len(set(native.EXPORTS)) == len(native.EXPORTS)
    assert callable(native.NativeContext.burst_runs) and callable(InpaintingEngine.find_burst_runs)
    api = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "api.hip")).read()
    assert re.search(r"^int si_burst_runs\(", api, re.M)
    kern = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "detect_kernels.hip")).read()
    route = kern[kern.index("    case SI_DET_BURST: {"):kern.index("    case SI_DET_INVALID:")]      # the route's pass 1 in the launcher's one switch
    assert "detect_burst_kernel" in kern and "detect_burst_kernel<T><<<" in route and re.findall(r'"(\w+)"', route) == ["detect_dead"]
    assert '"detect_burst"' not in kern                                 # profiled as "detect_dead": tests/poison.py's family lists are closed
    body = kern[kern.index("void bu_square(float"):kern.index("void bu_square(int16_t")]
    assert "#pragma clang fp contract(off)" in body and "fma" not in body.lower().replace("fused multiply", "")
    if os.path.exists(native.LIB_PATH):
        lib = native.load_library()
        assert lib.si_version() == 3 and len(lib.si_burst_runs.argtypes) == len(args) == 15
        assert list(lib.si_burst_runs.argtypes) == list(lib.si_level_runs.argtypes)


# ------------------------------------------------------------------------------------------------------------ predict.yaml
def _yaml(tmp_path, extra, drop=("mask",)):
    data = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "iea_predict.yaml")))
    for key in drop:
        data.pop(key, None)
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_kind_burst(tmp_path):
    defaults = {"threshold": 0.0, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0}
    cfg = load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: burst, threshold: 1.15, win_ms: 4.0}\n"))
    assert cfg.detect == {**defaults, "threshold": 1.15} and cfg.detect_dead == {"kind": "burst", "rel_threshold": 0.0, "held_tol": 0.0}
    assert cfg.detect_level == {"win_ms": 4.0}
    cfg = load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: burst, threshold: 1.15}\n"))
    assert cfg.detect_level == {"win_ms": 4.0}                           # the documented starting point is this kind's default window
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file}\ndetect: {kind: burst, win_ms: 8.5, rel_threshold: 2.5, channels: joint}\n"))
    assert cfg.detect == defaults and cfg.detect_level == {"win_ms": 8.5} and cfg.detect_dead["rel_threshold"] == 2.5 and cfg.detect_channels == "joint"
    assert load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: burst, rel_threshold: 4}\n")).detect_dead["rel_threshold"] == 4.0
    # every other kind keeps its shapes, defaults and limits
    cfg = load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {}\n"))
    assert cfg.detect == defaults and cfg.detect_dead == {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0} and cfg.detect_level == {"win_ms": 2.0}
    assert load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: level}\n")).detect_level == {"win_ms": 2.0}
    for kind in ("quiet", "held", "any", "level"):
        with pytest.raises(ValueError, match="detect.rel_threshold = 1.5 is a fraction of the file's peak, at most 1"):
            load_predict_config(_yaml(tmp_path, f"long: {{}}\ndetect: {{kind: {kind}, rel_threshold: 1.5}}\n"))
    with pytest.raises(ValueError, match="detect.rel_threshold = 4.5 is a fraction of the file's peak, at most 4 with `kind: burst`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: burst, rel_threshold: 4.5}\n"))
    with pytest.raises(ValueError, match="detect.held_tol = 0.001 with `kind: burst`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: burst, held_tol: 0.001}\n"))
    for bad in ("-1", ".nan", ".inf"):
        with pytest.raises(ValueError, match="detect.win_ms = .* is negative or not finite"):
            load_predict_config(_yaml(tmp_path, f"long: {{}}\ndetect: {{kind: burst, win_ms: {bad}}}\n"))
    with pytest.raises(ValueError, match=r"detect.kind = 'click': quiet .* or level .*, or burst \(the RMS level of the second difference"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: click}\n"))
    with pytest.raises(ValueError, match="unknown key `win` in `detect:`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: burst, win: 2}\n"))


# ------------------------------------------------------------------------------------------------------------ routing
class _Recorder:
    """Stands in for an engine under find_gaps: records which detector was called and with what."""
    DEAD_KINDS = InpaintingEngine.DEAD_KINDS
    ROWS = torch.tensor([[441 * 10, 441 * 3]], dtype=torch.int32)

    def __init__(self):
        self.calls = []

    def find_quiet_runs(self, *a, **kw):
        self.calls.append(("quiet", a[1:], kw))
        return self.ROWS

    def find_dead_runs(self, *a, **kw):
        self.calls.append(("dead", a[1:], kw))
        return self.ROWS, 0.125

    def find_level_runs(self, *a, **kw):
        self.calls.append(("level", a[1:], kw))
        return self.ROWS, 0.25

    def find_burst_runs(self, *a, **kw):
        self.calls.append(("burst", a[1:], kw))
        return self.ROWS, 1.15


def test_find_gaps_routes_kind_burst_and_nothing_else_to_the_burst_detector():
    x = torch.zeros(22050)
    rec = _Recorder()
    out = InpaintingEngine.find_gaps(rec, x, threshold=1.15, min_ms=5.0, kind="burst", win_ms=4.0)
    assert rec.calls == [("burst", (), dict(half=44, threshold=1.15, rel_threshold=0.0, min_len=110, channel=None, return_threshold=True))]
    assert sorted(out) == ["gaps", "runs", "skipped", "threshold"] and out["gaps"] == [(10, 3)] and out["threshold"] == 1.15
    rec.calls.clear()
    InpaintingEngine.find_gaps(rec, x.reshape(-1, 2), 48000, 0.0, kind="burst", rel_threshold=4.0, win_ms=3.0, channel=-1)
    assert rec.calls == [("burst", (), dict(half=72, threshold=0.0, rel_threshold=4.0, min_len=240, channel=-1, return_threshold=True))]
    rec.calls.clear()
    with pytest.raises(ValueError, match="held_tol = 0.5 with kind = 'burst'"):
        InpaintingEngine.find_gaps(rec, x, threshold=1.15, kind="burst", held_tol=0.5)
    with pytest.raises(ValueError, match="at most win_ms = 92.879 at this rate"):
        InpaintingEngine.find_gaps(rec, x, threshold=1.15, kind="burst", win_ms=100.0)
    for rel in (4.5, -0.5, float("nan")):
        with pytest.raises(ValueError, match=r"with kind = 'burst' is NaN or outside \[0, 4\]"):
            InpaintingEngine.find_gaps(rec, x, threshold=1.15, kind="burst", rel_threshold=rel)
    # T = 0: every window would be hot.  Refused before any call, with the starting point in the message
    with pytest.raises(ValueError, match=r"kind = 'burst' with threshold = 0 and rel_threshold = 0 is T = 0: every window would be hot.*"
                                         r"1\.15 of full scale.*win_ms = 4\.0"):
        InpaintingEngine.find_gaps(rec, x, kind="burst")
    assert rec.calls == []
    # every other kind is called as it was: no new keyword, whatever win_ms says
    InpaintingEngine.find_gaps(rec, x, threshold=0.01, win_ms=7.0)
    InpaintingEngine.find_gaps(rec, x, threshold=0.01, kind="held", win_ms=7.0)
    InpaintingEngine.find_gaps(rec, x, threshold=0.01, kind="level")
    assert rec.calls == [("quiet", (0.01, 110), {"channel": None}),
                         ("dead", ("held", 0.01, 0.0, 0.0, 110), {"channel": None, "return_threshold": True}),
                         ("level", (), dict(half=22, threshold=0.01, rel_threshold=0.0, min_len=110, channel=None, return_threshold=True))]


def test_conceal_routes_pass_win_ms_with_kind_burst():
    calls = []

    def find_gaps(*a, **kw):
        calls.append(kw)
        return {"gaps": [], "skipped": [], "runs": None, "threshold": 0.5}

    patched = lambda *a, **kw: {"patched": torch.zeros(4)}
    eng = types.SimpleNamespace(device=torch.device("cpu"), recording_frames=lambda *a: (100, 100), find_gaps=find_gaps, patch_file=patched,
                                patch_recording=patched)
    x = torch.zeros(48000)
    out = InpaintingEngine.conceal_file(eng, x, 48000, 1.15, kind="burst", win_ms=4.0)
    assert calls[-1] == {"channel": None, "kind": "burst", "rel_threshold": 0.0, "held_tol": 0.0, "win_ms": 4.0} and out["threshold"] == 0.5
    InpaintingEngine.conceal_file(eng, x.reshape(-1, 2), 48000, 1.15, kind="burst", win_ms=4.0, detect="each")
    assert [c["channel"] for c in calls[-2:]] == [0, 1] and all(c["win_ms"] == 4.0 for c in calls[-2:])
    InpaintingEngine.conceal_recording(eng, x[:22050], threshold=1.15, kind="burst", win_ms=6.0, rel_threshold=2.0)
    assert calls[-1] == {"kind": "burst", "rel_threshold": 2.0, "held_tol": 0.0, "win_ms": 6.0}
    # the calls of before
    InpaintingEngine.conceal_file(eng, x, 48000, 0.25, kind="any", win_ms=3.0)
    assert calls[-1] == {"channel": None, "kind": "any", "rel_threshold": 0.0, "held_tol": 0.0}
    InpaintingEngine.conceal_file(eng, x, 48000, 0.25, kind="level")
    assert calls[-1] == {"channel": None, "kind": "level", "rel_threshold": 0.0, "held_tol": 0.0, "win_ms": 2.0}
    InpaintingEngine.conceal_recording(eng, x[:22050], win_ms=1.0)
    assert calls[-1] == {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0}
    # the signatures and defaults did not change
    import inspect
    for fn in (InpaintingEngine.find_gaps, InpaintingEngine.conceal_file, InpaintingEngine.conceal_recording):
        p = inspect.signature(fn).parameters
        assert (p["kind"].default, p["rel_threshold"].default, p["held_tol"].default, p["win_ms"].default, p["threshold"].default) == ("quiet", 0.0, 0.0, 2.0, 0.0)


def test_find_burst_runs_checks_its_window_and_range_before_the_device():
    eng = types.SimpleNamespace()
    for kw, msg in ((dict(), "win = its odd length"), (dict(win=5, half=2), "not both"), (dict(win=4), "win = 4: an odd number"), (dict(win=0), "win = 0"),
                    (dict(half=-1), "half = -1 samples, outside 0 .. 1024"), (dict(half=1025), "half = 1025 samples"), (dict(win=2051), "half = 1025"),
                    (dict(half=1.5), "half = 1.5"), (dict(half=1, rel_threshold=4.0001), r"rel_threshold = 4.0001 is NaN or outside \[0, 4\]"),
                    (dict(half=1, rel_threshold=-1e-9), r"outside \[0, 4\]"), (dict(half=1, rel_threshold=float("nan")), r"is NaN or outside \[0, 4\]")):
        with pytest.raises(ValueError, match=msg):
            InpaintingEngine.find_burst_runs(eng, np.zeros(8, np.float32), **kw)


# ------------------------------------------------------------------------------------------------------------ PCM scaling
def test_the_threshold_is_scaled_for_a_pcm_file_and_win_ms_is_not(tmp_path, capsys):
    burst = types.SimpleNamespace(detect_dead={"kind": "burst", "rel_threshold": 0.0, "held_tol": 0.0}, detect_level={"win_ms": 4.0})
    assert P.level_keywords(burst) == {"win_ms": 4.0}
    assert P.level_keywords(types.SimpleNamespace(detect_dead={"kind": "any", "rel_threshold": 0.0, "held_tol": 0.0}, detect_level={"win_ms": 3.0})) == {}
    from scipy.io import wavfile
    calls = []

    def find_gaps(x, sr, thr, *a, **kw):
        calls.append((x.dtype, tuple(x.shape), thr, kw))
        if thr == 0.0 and kw["rel_threshold"] == 0.0:
            raise ValueError("find_gaps: kind = 'burst' with threshold = 0 and rel_threshold = 0 is T = 0")
        return {"gaps": [(10, 3)], "skipped": [], "runs": None, "threshold": thr}

    engine = types.SimpleNamespace(recording_frames=lambda n22, clip: (100, 100), find_gaps=find_gaps)
    pcm = (np.arange(22050) % 200 - 100).astype(np.int16)
    want_kw = {"kind": "burst", "rel_threshold": 0.0, "held_tol": 0.0, "win_ms": 4.0}
    for name, data, T, unit in (("pcm.wav", pcm, 1.25 * 32768, "int16 steps"), ("f32.wav", (pcm / 32768.0).astype(np.float32), 1.25, "full scale")):
        wavfile.write(tmp_path / name, 22050, data)
        cfg = types.SimpleNamespace(wave_path=str(tmp_path / name), detect={"threshold": 1.25, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0},
                                    detect_dead=burst.detect_dead, detect_level=burst.detect_level)
        assert P._detect_gaps(cfg, engine, data.astype(np.float32), 22050, 22050, 110, 200, 50, str(tmp_path)) == [(10, 3)]
        assert json.loads((tmp_path / "gaps.json").read_text()) == {"gaps": [[10, 3]], "skipped": [], "kind": "burst", "T": T, "win_ms": 4.0}
        assert f"Detection kind = burst, effective threshold T = {T} ({unit}), window win_ms = 4.0" in capsys.readouterr().out
    assert calls[0] == (np.int16, (22050,), 1.25 * 32768, want_kw) and calls[1] == (np.float32, (22050,), 1.25, want_kw)
    # packed 24-bit: 24-bit steps
    x24 = np.zeros((22050, 3), np.uint8)
    P._detect_gaps(cfg, engine, pcm.astype(np.float32), 22050, 22050, 110, 200, 50, str(tmp_path), x24=x24)
    assert calls[-1] == (np.uint8, (22050, 3), 1.25 * 8388608, want_kw)
    assert json.loads((tmp_path / "gaps.json").read_text()) == {"gaps": [[10, 3]], "skipped": [], "kind": "burst", "T": 1.25 * 8388608, "unit": "24-bit steps",
                                                                 "win_ms": 4.0}
    # the CLI hands on the engine's T = 0 refusal
    cfg.detect = {**cfg.detect, "threshold": 0.0}
    with pytest.raises(ValueError, match="is T = 0"):
        P._detect_gaps(cfg, engine, pcm.astype(np.float32), 22050, 22050, 110, 200, 50, str(tmp_path))
