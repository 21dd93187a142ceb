"""NaN, inf and out-of-range samples, the parts that need no GPU: the four declarations and their bindings, the
profile names of the new launchers, `kind: invalid` in predict.yaml with its defaults and refusals, the routing of kind="invalid"
through find_gaps, conceal_recording and conceal_file -- and of every other kind as before --, the ceiling on its way to patch_file and
patch_recording, its PCM scaling, and runs_to_gaps on a run of one sample."""
import inspect
import json
import math
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
from tests import poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("si_invalid_runs", "si_cut_rate_valid", "si_cut_pair_valid", "si_cut_clips_valid")
INF = float("inf")


# ------------------------------------------------------------------------------------------------------------ ABI
def _declaration(hdr, name):
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return [a.strip() for a in re.search(rf"^int {name}\((.*?)\);", code, flags=re.S | re.M).group(1).replace("\n", " ").split(",")]


def test_the_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "si_hip.h")).read()
    assert re.search(r"#define SI_ABI_VERSION 3\b", hdr)
    names = lambda args: [a.split()[-1].lstrip("*") for a in args]
    decl = {n: _declaration(hdr, n) for n in NEW}
    assert names(decl["si_invalid_runs"]) == ["ctx", "x", "is_pcm16", "n", "channels", "channel", "ceiling", "min_len", "runs", "max_runs", "n_runs", "stream"]
    # the mirrored calls' lists with channels / channel behind n_file (si_dead_runs' convention) and the ceiling in front of the outputs
    rate, pair, clips = (names(_declaration(hdr, n)) for n in ("si_cut_rate_ch", "si_cut_pair_ch", "si_cut_clips"))
    assert names(decl["si_cut_rate_valid"]) == rate[:-2] + ["ceiling"] + rate[-2:]
    assert names(decl["si_cut_pair_valid"]) == pair[:-3] + ["ceiling"] + pair[-3:]
    assert names(decl["si_cut_clips_valid"]) == clips[:-2] + ["ceiling"] + clips[-2:]
    for n in NEW:
        assert "float ceiling" in decl[n], n
    assert len(set(native.EXPORTS)) == len(native.EXPORTS) and all(n in native.EXPORTS for n in NEW)
    for fn in ("invalid_runs", "cut_rate_valid", "cut_pair_valid", "cut_clips_valid"):
        assert callable(getattr(native.NativeContext, fn))
    assert callable(InpaintingEngine.find_invalid_runs)
    # the header says what the entries stand for and counts the file-typed calls
    assert re.search(r"si_invalid_runs\s+<- nothing the reference computes", hdr) and "I_ea/predict.py:85-90" in hdr[hdr.index("si_invalid_runs      <-"):][:600]
    assert "The sixteen calls that take a file" in hdr and "The twelve calls" not in hdr
    doc = hdr[hdr.index("NaN, inf and out-of-range samples"):hdr.index("int si_invalid_runs(")]
    for phrase in ("DESIGN.md 4.30", "!(|v| <= min(c, FLT_MAX))", "-0.0 and subnormals are valid", "|-32768| = 32768", "24-bit steps", "c = 32766",
                   "no pass 0", "no threshold_out", "STAGED AS +0.0", "byte for byte", "SI_EINVAL before any launch", "<= 0 or NaN", "no atomics"):
        assert phrase in doc, phrase
    api = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "api.hip")).read()
    for n in NEW:
        assert re.search(rf"^int {n}\(", api, re.M), n
    # one definition of the predicate, used by the detector and the three feeds
    common = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "common.h")).read()
    assert common.count("bool si_invalid(") == 3 and "__builtin_fminf(c, __FLT_MAX__)" in common
    src = {f: open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", f)).read() for f in ("detect_kernels.hip", "rate_feed_kernels.hip", "patch_kernels.hip")}
    assert all("si_invalid(" in s and "bool si_invalid" not in s for s in src.values())
    assert "case SI_DET_INVALID:" in src["detect_kernels.hip"] and "rf_cut_tile<T, CLEAN>" in src["rate_feed_kernels.hip"] and "rf_pair_tile<T, CLEAN>" in src["rate_feed_kernels.hip"]
    assert src["rate_feed_kernels.hip"].count("si_with_flag(ceiling != nullptr, [&](auto clean)") == 2 and "cut_clips_kernel<decltype(clean)::value>" in src["patch_kernels.hip"]
    if os.path.exists(native.LIB_PATH):
        lib = native.load_library()
        assert lib.si_version() == 3
        for n in NEW:
            argtypes = getattr(lib, n).argtypes
            assert len(argtypes) == len(decl[n]), n
            assert [t is native.C.c_float for t in argtypes] == [a == "float ceiling" for a in decl[n]], n


def test_the_new_launchers_use_profile_names_of_the_closed_lists():
    """Every si_prof_begin of the new launchers names a family tests/poison.py already has: detect_bits[_ch] with scratch, the cutters
    without."""
    families = set(poison.SCRATCH_FAMILIES) | set(poison.NO_SCRATCH_FAMILIES)
    found = set()
    for f in ("detect_kernels.hip", "rate_feed_kernels.hip", "patch_kernels.hip"):
        src = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", f)).read()
        for name in re.findall(r'si_prof_begin\(ctx, (.*?), [0-9a-z]', src):
            for lit in re.findall(r'"(\w+)"', name):
                found.add(lit)
                assert lit in families, (f, lit)
    assert {"detect_bits", "detect_bits_ch", "cut_rate", "cut_rate_ch", "cut_clips"} <= found
    kern = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "detect_kernels.hip")).read()
    body = kern[kern.index("    case SI_DET_INVALID:"):kern.index("    case SI_DET_IMPULSE: {")]     # the route's case of the launcher's one switch
    assert "detect_invalid_kernel<T><<<" in body and "detect_invalid_ch_kernel<T><<<" in body
    assert re.findall(r'"(\w+)"', body) == ["detect_bits", "detect_bits_ch"] and "detect_invalid" not in "".join(re.findall(r'"(\w+)"', kern))
    assert "detect_bits" in poison.SCRATCH_FAMILIES and "cut_rate" in poison.NO_SCRATCH_FAMILIES and "cut_clips" in poison.NO_SCRATCH_FAMILIES


# ------------------------------------------------------------------------------------------------------------ predict.yaml
def _yaml(tmp_path, extra, drop=("mask",)):
    data = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "iea_predict.yaml")))
    for key in drop:
        data.pop(key, None)
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_kind_invalid(tmp_path):
    defaults = {"threshold": 0.0, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0}
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file, feed: contexts}\ndetect: {kind: invalid}\n"))
    assert cfg.detect == {**defaults, "min_ms": 0.0} and cfg.detect_dead == {"kind": "invalid", "rel_threshold": 0.0, "held_tol": 0.0}
    assert cfg.detect_level == {"win_ms": 2.0} and cfg.detect_channels == "each"                    # the shapes of before
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file, feed: contexts}\ndetect: {kind: invalid, threshold: 1.5, min_ms: 2.0, channels: joint}\n"))
    assert cfg.detect == {**defaults, "threshold": 1.5, "min_ms": 2.0} and cfg.detect_channels == "joint"
    # min_ms is 0 at this kind only
    for kind in ("quiet", "held", "any", "level", "burst"):
        assert load_predict_config(_yaml(tmp_path, f"long: {{}}\ndetect: {{kind: {kind}, threshold: 1.15}}\n")).detect["min_ms"] == 5.0
    assert load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {}\n")).detect == defaults
    for key in ("rel_threshold", "held_tol"):
        with pytest.raises(ValueError, match=rf"detect.{key} = 0.5 with `kind: invalid`"):
            load_predict_config(_yaml(tmp_path, f"long: {{}}\ndetect: {{kind: invalid, {key}: 0.5}}\n"))
        assert load_predict_config(_yaml(tmp_path, f"long: {{}}\ndetect: {{kind: invalid, {key}: 0}}\n")).detect_dead[key] == 0.0
    with pytest.raises(ValueError, match=r"detect.win_ms needs `kind: level` \(kind: invalid judges sample by sample and has no window\)"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: invalid, win_ms: 2.0}\n"))
    # the two messages existing tests match keep their wording as a prefix; the kind list ends with the new kind
    with pytest.raises(ValueError, match=r"detect.kind = 'click': quiet .* or level .*, or burst \(the RMS level of the second difference over a window of "
                                         r"win_ms milliseconds >= the threshold\), or invalid \("):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: click}\n"))
    with pytest.raises(ValueError, match=r"detect.win_ms needs `kind: level` \(kind: held judges sample by sample and has no window\)$"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: held, win_ms: 2.0}\n"))
    with pytest.raises(ValueError, match=r"unknown key `ceiling` in `detect:` \(it takes threshold, min_ms, max_ms, pad_frames, channels, kind, rel_threshold, "
                                         r"held_tol\) and, with kind: level, win_ms \(kind: burst takes it too\)$"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: invalid, ceiling: 2}\n"))
    with pytest.raises(ValueError, match="detect.threshold = -1.0 is negative"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: invalid, threshold: -1}\n"))


# ------------------------------------------------------------------------------------------------------------ routing
class _Recorder:
    """Stands in for an engine under find_gaps: records which detector was called and with what."""
    DEAD_KINDS = InpaintingEngine.DEAD_KINDS
    ROWS = torch.tensor([[441 * 10, 1]], dtype=torch.int32)

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

    def find_invalid_runs(self, *a, **kw):
        self.calls.append(("invalid", a[1:], kw))
        return self.ROWS


def test_find_gaps_routes_kind_invalid_and_nothing_else_to_the_invalid_detector():
    x = torch.zeros(22050)
    rec = _Recorder()
    out = InpaintingEngine.find_gaps(rec, x, min_ms=0, kind="invalid")
    assert rec.calls == [("invalid", (), dict(ceiling=INF, min_len=1, channel=None))]                 # threshold = 0: no ceiling
    assert sorted(out) == ["gaps", "runs", "skipped", "threshold"] and out["gaps"] == [(10, 1)] and out["threshold"] == INF
    rec.calls.clear()
    out = InpaintingEngine.find_gaps(rec, x.reshape(-1, 2), 48000, 1.5, kind="invalid", channel=-1, win_ms=9.0)     # win_ms is not read
    assert rec.calls == [("invalid", (), dict(ceiling=1.5, min_len=240, channel=-1))] and out["threshold"] == 1.5   # min_ms keeps its default
    rec.calls.clear()
    with pytest.raises(ValueError, match=r"find_gaps: rel_threshold = 0.5 with kind = 'invalid' \(the ceiling is `threshold`"):
        InpaintingEngine.find_gaps(rec, x, kind="invalid", rel_threshold=0.5)
    with pytest.raises(ValueError, match=r"find_gaps: held_tol = 0.25 with kind = 'invalid' \(held samples are kind 'held' or 'any'\)"):
        InpaintingEngine.find_gaps(rec, x, kind="invalid", held_tol=0.25)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match=r"threshold = .* with kind = 'invalid' is negative or NaN"):
            InpaintingEngine.find_gaps(rec, x, threshold=bad, kind="invalid")
    assert rec.calls == []
    # every other kind is called as it was
    InpaintingEngine.find_gaps(rec, x, threshold=0.01)
    InpaintingEngine.find_gaps(rec, x, threshold=0.01, kind="held")
    InpaintingEngine.find_gaps(rec, x, threshold=0.01, kind="level")
    InpaintingEngine.find_gaps(rec, x, threshold=1.15, kind="burst", win_ms=4.0)
    assert rec.calls == [("quiet", (0.01, 110), {"channel": None}),
                         ("dead", ("held", 0.01, 0.0, 0.0, 110), {"channel": None, "return_threshold": True}),
                         ("level", (), dict(half=22, threshold=0.01, rel_threshold=0.0, min_len=110, channel=None, return_threshold=True)),
                         ("burst", (), dict(half=44, threshold=1.15, rel_threshold=0.0, min_len=110, channel=None, return_threshold=True))]


def test_find_invalid_runs_refuses_a_bad_ceiling_before_the_device():
    eng = types.SimpleNamespace()
    for bad in (0.0, -1.0, float("nan"), -INF):
        with pytest.raises(ValueError, match=r"find_invalid_runs: ceiling = .* is not above 0, or is NaN"):
            InpaintingEngine.find_invalid_runs(eng, np.zeros(8, np.float32), ceiling=bad)
    p = inspect.signature(InpaintingEngine.find_invalid_runs).parameters
    assert [(k, v.default) for k, v in p.items()][2:] == [("ceiling", INF), ("min_len", 1), ("max_runs", 65536), ("channel", None)]
    assert G.invalid_ceiling(0) == INF and G.invalid_ceiling(0.0) == INF and G.invalid_ceiling(32766) == 32766.0 and G.invalid_ceiling(INF) == INF


def test_conceal_routes_pass_the_ceiling_at_kind_invalid_only():
    finds, patches = [], []

    def find_gaps(*a, **kw):
        finds.append(kw)
        return {"gaps": [], "skipped": [], "runs": None, **({"threshold": 0.5} if kw["kind"] != "quiet" else {})}

    def patched(*a, **kw):
        patches.append(kw)
        return {"patched": torch.zeros(4)}

    eng = types.SimpleNamespace(device=torch.device("cpu"), recording_frames=lambda *a: (100, 100), find_gaps=find_gaps, patch_file=patched,
                                patch_recording=patched)
    x = torch.zeros(48000)
    base_file = dict(fade_ms=5.0, clip_frames=200, min_context=50, batch=32, return_windows=False)
    out = InpaintingEngine.conceal_file(eng, x, 48000, min_ms=0, kind="invalid", feed="contexts")
    assert finds[-1] == {"channel": None, "kind": "invalid", "rel_threshold": 0.0, "held_tol": 0.0}                 # no win_ms
    assert patches[-1] == {**base_file, "feed": "contexts", "ceiling": INF} and out["threshold"] == 0.5
    InpaintingEngine.conceal_file(eng, x, 48000, 2.5, min_ms=0, kind="invalid", feed="contexts", clips16="file")
    assert patches[-1] == {**base_file, "feed": "contexts", "clips16": "file", "ceiling": 2.5}
    InpaintingEngine.conceal_file(eng, x.reshape(-1, 2), 48000, 32766.0, min_ms=0, kind="invalid", feed="contexts", detect="each")
    assert [c["channel"] for c in finds[-2:]] == [0, 1] and patches[-1]["ceiling"] == 32766.0 and "channel_gaps" in patches[-1]
    base_rec = dict(wave16=None, fade=110, clip_frames=200, min_context=50, batch=32, pcm=False)
    InpaintingEngine.conceal_recording(eng, x[:22050], min_ms=0, kind="invalid")
    assert finds[-1] == {"kind": "invalid", "rel_threshold": 0.0, "held_tol": 0.0} and patches[-1] == {**base_rec, "ceiling": INF}
    InpaintingEngine.conceal_recording(eng, x[:22050], threshold=1.0, min_ms=0, kind="invalid")
    assert patches[-1] == {**base_rec, "ceiling": 1.0}
    with pytest.raises(ValueError, match=r"conceal_recording: kind = 'invalid' with detect_on: the samples that are fed .* must be the ones that were judged"):
        InpaintingEngine.conceal_recording(eng, x[:22050], detect_on=x, sr=48000, kind="invalid")
    # every other kind hands on no new keyword
    n = len(patches)
    for kind, kw in (("quiet", {}), ("held", {}), ("any", {}), ("level", {}), ("burst", {"win_ms": 4.0})):
        InpaintingEngine.conceal_file(eng, x, 48000, 1.15, kind=kind, **kw)
        assert patches[-1] == {**base_file, "feed": "recording"}, kind
        InpaintingEngine.conceal_recording(eng, x[:22050], threshold=1.15, kind=kind, **kw)
        assert patches[-1] == base_rec, kind
    assert len(patches) == n + 10
    # the signatures and defaults did not change; patch_* gained one keyword, None by default
    for fn in (InpaintingEngine.find_gaps, InpaintingEngine.conceal_file, InpaintingEngine.conceal_recording):
        p = inspect.signature(fn).parameters
        assert (p["kind"].default, p["rel_threshold"].default, p["held_tol"].default, p["win_ms"].default, p["threshold"].default, p["min_ms"].default) == \
            ("quiet", 0.0, 0.0, 2.0, 0.0, 5.0) and "ceiling" not in p
    for fn in (InpaintingEngine.patch_file, InpaintingEngine.patch_recording):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "ceiling" and p["ceiling"].default is None


def _bare_engine():
    """An engine object with no context: enough for the refusals patch_file and patch_recording raise before they touch the device."""
    eng = InpaintingEngine.__new__(InpaintingEngine)
    eng._need = lambda **kw: None
    eng.device = torch.device("cpu")
    return eng


def test_patch_calls_refuse_a_bad_ceiling_and_the_recording_feed():
    eng = _bare_engine()
    x = np.zeros(48000, np.float32)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match=r"patch_file: ceiling = .* is not above 0, or is NaN"):
            eng.patch_file(x, 48000, [(10, 2)], feed="contexts", ceiling=bad)
        with pytest.raises(ValueError, match=r"patch_recording: ceiling = .* is not above 0, or is NaN"):
            eng.patch_recording(x[:22050], [(10, 2)], ceiling=bad)
    for feed_kw in ({}, {"feed": "recording"}):
        with pytest.raises(ValueError, match=r'patch_file: ceiling = inf needs feed="contexts" at 48000 Hz'):
            eng.patch_file(x, 48000, [(10, 2)], ceiling=INF, **feed_kw)
        with pytest.raises(ValueError, match=r'patch_file: ceiling = 1.0 needs feed="contexts" at 44100 Hz'):
            eng.patch_file(np.zeros((44100, 2), np.float32), 44100, [(10, 2)], ceiling=1.0, **feed_kw)
    assert InpaintingEngine._ceiling(None, "f") is None and InpaintingEngine._ceiling(INF, "f") == INF and InpaintingEngine._ceiling(3, "f") == 3.0


# ------------------------------------------------------------------------------------------------------------ the CLI
def test_the_ceiling_is_scaled_for_a_pcm_file_and_recorded(tmp_path, capsys):
    from scipy.io import wavfile
    dead = {"kind": "invalid", "rel_threshold": 0.0, "held_tol": 0.0}
    cfg = lambda thr: types.SimpleNamespace(detect={"threshold": thr, "min_ms": 0.0, "max_ms": 400.0, "pad_frames": 0}, detect_dead=dead, detect_level={"win_ms": 2.0})
    assert P.ceiling_keywords(cfg(0.0), 1.0) == {"ceiling": INF} and P.ceiling_keywords(cfg(0.0), 32768.0) == {"ceiling": INF}
    assert P.ceiling_keywords(cfg(1.5), 1.0) == {"ceiling": 1.5} and P.ceiling_keywords(cfg(0.75), 32768.0) == {"ceiling": 24576.0}
    assert P.ceiling_keywords(cfg(0.5), 8388608.0) == {"ceiling": 4194304.0}
    for kind in ("quiet", "held", "any", "level", "burst"):
        assert P.ceiling_keywords(types.SimpleNamespace(detect=cfg(1.0).detect, detect_dead={**dead, "kind": kind}), 1.0) == {}
    assert P.ceiling_keywords(types.SimpleNamespace(detect=None, detect_dead=None), 1.0) == {}
    assert P.level_keywords(cfg(0.0)) == {} and P.dead_keywords(dead, 32768.0) == dead
    calls = []

    def find_gaps(x, sr, thr, *a, **kw):
        calls.append((x.dtype, tuple(x.shape), thr, a[0], kw))
        return {"gaps": [(10, 1)], "skipped": [(0, 1, "edge")], "runs": None, "threshold": G.invalid_ceiling(thr)}

    engine = types.SimpleNamespace(recording_frames=lambda n22, clip: (100, 100), find_gaps=find_gaps)
    pcm = (np.arange(22050) % 200 - 100).astype(np.int16)
    for name, data, thr, want_thr, ceiling, unit in (("pcm.wav", pcm, 0.75, 24576.0, 24576.0, "int16 steps"),
                                                     ("f32.wav", (pcm / 32768.0).astype(np.float32), 0.0, 0.0, None, "full scale"),
                                                     ("f32.wav", (pcm / 32768.0).astype(np.float32), 1.5, 1.5, 1.5, "full scale")):
        wavfile.write(tmp_path / name, 22050, data)
        c = cfg(thr)
        c.wave_path = str(tmp_path / name)
        assert P._detect_gaps(c, engine, data.astype(np.float32), 22050, 22050, 110, 200, 50, str(tmp_path)) == [(10, 1)]
        assert calls[-1] == (data.dtype, (22050,), want_thr, 0.0, dead)                                   # min_ms = 0 reaches find_gaps
        text = (tmp_path / "gaps.json").read_text()
        assert "Infinity" not in text and "NaN" not in text                                              # strict JSON: no ceiling is null
        assert json.loads(text) == {"gaps": [[10, 1]], "skipped": [[0, 1, "edge"]], "kind": "invalid", "ceiling": ceiling}
        assert f"Detection kind = invalid, ceiling = {'none' if ceiling is None else ceiling} ({unit})" in capsys.readouterr().out
    x24 = np.zeros((22050, 3), np.uint8)
    P._detect_gaps(c, engine, pcm.astype(np.float32), 22050, 22050, 110, 200, 50, str(tmp_path), x24=x24)
    assert calls[-1][:3] == (np.uint8, (22050, 3), 1.5 * 8388608)
    assert json.loads((tmp_path / "gaps.json").read_text())["unit"] == "24-bit steps"


def test_the_cli_hands_the_ceiling_to_patch_file_and_the_engines_refusal_on(tmp_path):
    from scipy.io import wavfile
    x = (0.25 * np.sin(np.arange(48000) / 30.0)).astype(np.float32)
    x[24000] = np.nan
    wavfile.write(tmp_path / "f.wav", 48000, x)
    seen = []

    def patch_file(xx, sr, gaps, **kw):
        seen.append((sr, list(gaps), kw))
        if kw.get("ceiling") is not None and kw["feed"] != "contexts":
            raise ValueError('patch_file: ceiling = inf needs feed="contexts" at 48000 Hz')
        return {"patched": torch.from_numpy(np.nan_to_num(xx)), "labels": torch.zeros(1, dtype=torch.int64), "label_off": [0, 1]}

    engine = types.SimpleNamespace(recording_frames=lambda n22, clip: (50, 49), patch_file=patch_file,
                                   find_gaps=lambda *a, **kw: {"gaps": [(25, 1)], "skipped": [], "runs": None, "threshold": INF})
    mk = lambda feed: types.SimpleNamespace(wave_path=str(tmp_path / "f.wav"), long={"clip_s": 4.0, "context_s": 1.0, "batch": 32}, long_feed=feed,
                                            long_clips16="resampled", long_pcm24="float32", patch_fade_ms=None, gaps=None,
                                            detect={"threshold": 0.0, "min_ms": 0.0, "max_ms": 400.0, "pad_frames": 0},
                                            detect_dead={"kind": "invalid", "rel_threshold": 0.0, "held_tol": 0.0}, detect_level={"win_ms": 2.0})
    assert P._main_long_file(mk("contexts"), engine, str(tmp_path)) == 0
    assert seen[-1][0] == 48000 and seen[-1][1] == [(25, 1)] and seen[-1][2]["ceiling"] == INF and seen[-1][2]["feed"] == "contexts"
    assert json.loads((tmp_path / "gaps.json").read_text()) == {"gaps": [[25, 1]], "skipped": [], "kind": "invalid", "ceiling": None}
    with pytest.raises(ValueError, match=r'needs feed="contexts"'):
        P._main_long_file(mk("recording"), engine, str(tmp_path))
    # any other kind: patch_file is called as it was
    cfg = mk("contexts")
    cfg.detect_dead = {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0}
    engine.find_gaps = lambda *a, **kw: {"gaps": [(25, 1)], "skipped": [], "runs": None}
    P._main_long_file(cfg, engine, str(tmp_path))
    assert "ceiling" not in seen[-1][2]


# ------------------------------------------------------------------------------------------------------------ the grid
def test_runs_to_gaps_covers_a_run_of_one_sample_by_one_frame():
    for sr, n in ((48000, 480000), (22050, 220500), (44100, 441000), (8000, 80000), (11025, 110250)):
        per = sr / 50.0
        for s in (int(7 * per) + 1, int(8 * per) - 1 if per == int(per) else int(8 * per), 12345, n - 2):
            gaps, skipped = G.runs_to_gaps([(s, 1)], n, sr, n * 50 // sr, n * 50 // sr, 0, 2, 20)
            f = s * 50 // sr
            assert gaps == [(f, 1)] and skipped == [], (sr, s, gaps, skipped)
    # two single samples in neighbouring frames merge; a scatter inside one frame is one frame; sample 0 and sample n - 1 are edges
    assert G.runs_to_gaps([(960 * 5 + 3, 1), (960 * 6 + 900, 1)], 480000, 48000, 500, 500, 0, 2, 20) == ([(5, 2)], [])
    assert G.runs_to_gaps([(960 * 5 + k, 1) for k in (0, 7, 8, 500, 959)], 480000, 48000, 500, 500, 0, 2, 20) == ([(5, 1)], [])
    assert G.runs_to_gaps([(0, 1), (479999, 1)], 480000, 48000, 500, 500, 0, 2, 20) == ([], [(0, 1, "edge"), (499, 1, "edge")])
    assert math.isinf(G.invalid_ceiling(0))
