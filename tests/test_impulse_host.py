"""Clicks and pops by locally scaled AR prediction error, the parts that need no GPU: the two declarations and their
bindings, the profile name against the closed family lists, `kind: impulse` in predict.yaml with its keys, defaults and refusals, the
routing of kind="impulse" through find_gaps, conceal_recording and conceal_file -- and of every other kind as before, with no new
keyword --, win_ms -> half, and the PCM scaling on the way from predict.yaml to the engine."""
import inspect
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
from tests import poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ ABI
def test_the_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "si_hip.h")).read()
    assert re.search(r"#define SI_ABI_VERSION 3\b", hdr)
    m = re.search(r"^int si_impulse_runs\((.*?)\);", hdr, re.S | re.M)
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["si_ctx* ctx", "const void* x", "int is_pcm16", "int n", "int channels", "int channel", "int order", "int half", "int guard", "int pad",
                    "float ratio", "float threshold", "float rel_threshold", "int min_len", "int32_t* runs", "int max_runs", "int32_t* n_runs",
                    "float* threshold_out", "si_stream_t stream"]
    tap = re.search(r"^int si_impulse_residual\((.*?)\);", hdr, re.S | re.M).group(1).replace("\n", " ")
    assert [a.strip() for a in tap.split(",")] == ["si_ctx* ctx", "const void* x", "int is_pcm16", "int n", "int channels", "int channel", "int order",
                                                   "double* e", "si_stream_t stream"]
    doc = hdr[hdr.index("Clicks and pops by locally scaled AR prediction error"):m.start()]
    for phrase in ("The reference has no detection", "I_ea/predict.py:85-90", "max(threshold, fl32(rel_threshold * peak))", "T = 0\n *             is allowed",
                   "[max(0, b B - 256), min(n, (b + 1) B + 256))", "eight partial sums", "r[0] * (1 + 1e-9)", "Levinson-Durbin", "a = (1, 0, ..., 0)",
                   "counted with integers", "added in this order", "no fused multiply-add", "[max(p, t - h), t - g - 1]", "[t + g + 1, min(n - 1, t + h)]",
                   "BY ADDITIONS ONLY", "cnt * 2^-52 * S", "cnt(t) >= h - g", "There is no division", "|t - j| <= pad", "never the adjacent ones",
                   "EVERY channel's dead_c holds", "n <= p gives zero runs", "no atomics", "135 168 bytes", "ratio NaN or outside [1, 1e6]",
                   "rel_threshold NaN or outside [0, 4]", "0.0 for t < p, NaN for a bad sample", "same device functions"):
        assert phrase in doc, phrase
    assert re.search(r"si_impulse_runs, si_impulse_residual\s+<- nothing the reference computes", hdr)
    for name, value in (("ORDER", 32), ("HALF", 1024), ("GUARD", 64), ("PAD", 16)):
        assert re.search(rf"#define SI_IMPULSE_MAX_{name} {value}\b", hdr) and getattr(native, f"IMPULSE_MAX_{name}") == getattr(G, f"IMPULSE_MAX_{name}") == value
    assert {"si_impulse_runs", "si_impulse_residual"} <= set(native.EXPORTS) and len(set(native.EXPORTS)) == len(native.EXPORTS)
    assert callable(native.NativeContext.impulse_runs) and callable(native.NativeContext.impulse_residual)
    assert callable(InpaintingEngine.find_impulse_runs) and callable(InpaintingEngine.impulse_residual)
    api = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "api.hip")).read()
    assert re.search(r"^int si_impulse_runs\(", api, re.M) and re.search(r"^int si_impulse_residual\(", api, re.M)
    if os.path.exists(native.LIB_PATH):
        lib = native.load_library()
        assert lib.si_version() == 3 and len(lib.si_impulse_runs.argtypes) == len(args) == 19 and len(lib.si_impulse_residual.argtypes) == 9


def test_one_body_two_wrappers_and_a_profile_name_of_the_closed_lists():
    kern = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "detect_kernels.hip")).read()
    assert "case SI_DET_IMPULSE:" in kern and kern.count("im_residual_body(x, n, ch,") == 2      # the detector and the tap call the same body
    for name in ("detect_impulse_kernel", "detect_impulse_residual_kernel"):
        assert re.search(rf"__global__ __launch_bounds__\(256\) void {name}\(", kern)
    assert '"detect_impulse"' not in kern and "detect_dead" in poison.SCRATCH_FAMILIES
    families = set(poison.SCRATCH_FAMILIES) | set(poison.NO_SCRATCH_FAMILIES)
    # the launcher's pass 0, written once in front of its one switch, and the route's own case
    launcher = kern[kern.index("    if (d.rel > 0.f) {"):kern.index("    switch (d.route) {")] + kern[kern.index("    case SI_DET_IMPULSE: {"):kern.index("    default:")]
    assert "detect_impulse_kernel<T><<<" in launcher
    assert re.findall(r'si_prof_begin\(ctx, "(\w+)"', launcher) == ["detect_peak", "detect_peak_final", "detect_dead"]
    tap = kern[kern.index("static int im_residual_launch_t("):]
    assert re.findall(r'si_prof_begin\(ctx, "(\w+)"', tap) == ["detect_dead"] and {"detect_peak", "detect_peak_final", "detect_dead"} <= families
    body = kern[kern.index("void im_residual_body("):kern.index("void detect_impulse_kernel(")]
    assert "#pragma clang fp contract(off)" in body and "fma" not in body.lower() and "atomic" not in body.lower()
    sizes = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "detect_sizes.h")).read()
    assert "dt_impulse_lds" in sizes and "IM_MAX_HALF = 1024" in sizes
    check = open(os.path.join(ROOT, "tools", "detcheck_main.cpp")).read()
    assert "dt_impulse_lds" in check and "135168" in check


# ------------------------------------------------------------------------------------------------------------ predict.yaml
def _yaml(tmp_path, extra, drop=("mask",)):
    data = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "iea_predict.yaml")))
    for key in drop:
        data.pop(key, None)
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_kind_impulse(tmp_path):
    assert G.IMPULSE_DEFAULTS == dict(order=16, win_ms=23.0, guard=4, pad=2, ratio=10.0)
    defaults = {"threshold": 0.0, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0}
    cfg = load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: impulse}\n"))
    assert cfg.detect == defaults and cfg.detect_dead == {"kind": "impulse", "rel_threshold": 0.0, "held_tol": 0.0}
    assert cfg.detect_level == {"win_ms": 23.0} and cfg.detect_impulse == {"ratio": 10.0, "order": 16, "guard": 4, "pad": 2} and cfg.detect_mend is None
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file}\ndetect: {kind: impulse, ratio: 12, order: 24, guard: 6, pad: 3, win_ms: 11.5, threshold: 0.01, "
                                              "rel_threshold: 2.5, min_ms: 0, mend_ms: 1, channels: joint}\n"))
    assert cfg.detect == {**defaults, "threshold": 0.01, "min_ms": 0.0} and cfg.detect_level == {"win_ms": 11.5}
    assert cfg.detect_impulse == {"ratio": 12.0, "order": 24, "guard": 6, "pad": 3} and cfg.detect_dead["rel_threshold"] == 2.5
    assert cfg.detect_mend == {"mend_ms": 1.0, "mend_order": 32, "mend_context": 512} and cfg.detect_channels == "joint"
    # absent keys leave the parse result as it is: every other kind has no detect_impulse, and its window default
    for kind, win in (("quiet", 2.0), ("held", 2.0), ("any", 2.0), ("level", 2.0), ("burst", 4.0), ("invalid", 2.0)):
        cfg = load_predict_config(_yaml(tmp_path, f"long: {{}}\ndetect: {{kind: {kind}}}\n"))
        assert cfg.detect_impulse is None and cfg.detect_level == {"win_ms": win}, kind
        for key in ("ratio", "order", "guard", "pad"):
            with pytest.raises(ValueError, match=f"detect.{key} needs `kind: impulse` \\(kind: {kind} has no prediction-error test\\)"):
                load_predict_config(_yaml(tmp_path, f"long: {{}}\ndetect: {{kind: {kind}, {key}: 3}}\n"))
    assert load_predict_config(_yaml(tmp_path, "long: {}\n")).detect_impulse is None
    for text, msg in (("ratio: 0.5", r"detect.ratio = 0.5 is NaN or outside \[1, 1e6\] \(10 is the default\)"), ("ratio: .nan", r"detect.ratio = nan is NaN or outside"),
                      ("ratio: 2.0e+6", r"detect.ratio = 2000000.0 is NaN or outside"), ("order: 1", r"detect.order = 1, outside 2 .. 32 \(16 is the default\)"),
                      ("order: 33", "detect.order = 33, outside 2 .. 32"), ("order: 2.5", "detect.order = 2.5: a whole number"),
                      ("guard: -1", r"detect.guard = -1 samples, outside 0 .. 64 \(4 is the default\)"), ("guard: 65", "detect.guard = 65 samples, outside 0 .. 64"),
                      ("pad: -1", r"detect.pad = -1 samples, outside 0 .. 16 \(2 is the default\)"), ("pad: 17", "detect.pad = 17 samples, outside 0 .. 16"),
                      ("rel_threshold: 4.5", "detect.rel_threshold = 4.5 is a fraction of the file's peak, at most 4 with `kind: impulse`"),
                      ("held_tol: 0.001", "detect.held_tol = 0.001 with `kind: impulse`"), ("win_ms: -1", "detect.win_ms = -1.0 is negative or not finite"),
                      ("win: 2", "unknown key `win` in `detect:`")):
        with pytest.raises(ValueError, match=msg):
            load_predict_config(_yaml(tmp_path, f"long: {{}}\ndetect: {{kind: impulse, {text}}}\n"))
    with pytest.raises(ValueError, match="detect.mend_ms needs `long: {rate: file}`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: impulse, min_ms: 0, mend_ms: 1}\n"))
    # the unknown-kind message keeps its wording as a prefix and ends with the new kind
    with pytest.raises(ValueError, match=r"detect.kind = 'click': quiet .* or level .*, or burst \(the RMS level of the second difference.*"
                                         r"or invalid \(NaN, inf and \|x\| > the threshold, the ceiling; 0 = no ceiling\), or impulse \(.*\)$"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: click}\n"))


# ------------------------------------------------------------------------------------------------------------ routing
class _Recorder:
    """Stands in for an engine under find_gaps: records which detector was called and with what."""
    DEAD_KINDS = InpaintingEngine.DEAD_KINDS
    ROWS = torch.tensor([[441 * 10, 441 * 3]], dtype=torch.int32)

    def __init__(self):
        self.calls = []

    def _note(self, name, T=None):
        def call(*a, **kw):
            self.calls.append((name, a[1:], kw))
            return self.ROWS if T is None else (self.ROWS, T)
        return call

    def __getattr__(self, name):
        table = {"find_quiet_runs": ("quiet", None), "find_dead_runs": ("dead", 0.125), "find_level_runs": ("level", 0.25),
                 "find_burst_runs": ("burst", 1.15), "find_invalid_runs": ("invalid", None), "find_impulse_runs": ("impulse", 0.0)}
        if name in table:
            return self._note(*table[name])
        raise AttributeError(name)


def test_find_gaps_routes_kind_impulse_and_nothing_else_to_the_impulse_detector():
    x = torch.zeros(22050)
    rec = _Recorder()
    out = InpaintingEngine.find_gaps(rec, x, min_ms=0, kind="impulse")
    assert rec.calls == [("impulse", (), dict(half=254, order=16, guard=4, pad=2, ratio=10.0, threshold=0.0, rel_threshold=0.0, min_len=1, channel=None,
                                               return_threshold=True))]                      # win_ms = 23 at 22.05 kHz: half = round(253.575)
    assert sorted(out) == ["gaps", "runs", "skipped", "threshold"] and out["threshold"] == 0.0
    rec.calls.clear()
    InpaintingEngine.find_gaps(rec, x.reshape(-1, 2), 48000, 0.02, kind="impulse", rel_threshold=4.0, win_ms=10.0, channel=-1, impulse_order=24, impulse_guard=6,
                               impulse_pad=3, impulse_ratio=12.0)
    assert rec.calls == [("impulse", (), dict(half=240, order=24, guard=6, pad=3, ratio=12.0, threshold=0.02, rel_threshold=4.0, min_len=240, channel=-1,
                                               return_threshold=True))]
    rec.calls.clear()
    assert G.level_half(23.0, 48000) == 552 and G.level_half(23.0, 8000) == 92 and G.level_half(2.0, 22050) == 22
    for kw, msg in ((dict(held_tol=0.5), "held_tol = 0.5 with kind = 'impulse'"), (dict(win_ms=100.0), "at most win_ms = 92.879 at this rate"),
                    (dict(win_ms=0.3), r"half = 3 samples \(win_ms = 0.3 at 22050 Hz\) is under guard \+ 1 = 5.*raise win_ms to 0.454 or more, or lower guard"),
                    (dict(win_ms=92.8), r"half \+ pad = 1025 samples \(win_ms = 92.8 at 22050 Hz\), above 1024: lower win_ms to 92.698 or less"),
                    (dict(impulse_order=1), "order = 1, outside 2 .. 32: 16 is the default"), (dict(impulse_order=33), "order = 33, outside 2 .. 32"),
                    (dict(impulse_guard=65), "guard = 65 samples, outside 0 .. 64: 4 is the default"), (dict(impulse_pad=17), "pad = 17 samples, outside 0 .. 16: 2 is the default"),
                    (dict(impulse_ratio=0.5), r"ratio = 0.5 is NaN or outside \[1, 1e6\]"), (dict(impulse_ratio=float("nan")), r"ratio = nan is NaN or outside \[1, 1e6\]"),
                    (dict(rel_threshold=4.5), r"rel_threshold = 4.5 is NaN or outside \[0, 4\]")):
        with pytest.raises(ValueError, match=msg) as err:
            InpaintingEngine.find_gaps(rec, x, kind="impulse", **kw)
        assert str(err.value).startswith("find_gaps: ") or "win_ms" in kw        # gaps.level_half speaks for itself
    assert rec.calls == []
    # every other kind is called as it was: no new keyword, whatever the impulse_* keywords say
    odd = dict(impulse_order=3, impulse_guard=1, impulse_pad=9, impulse_ratio=77.0)
    InpaintingEngine.find_gaps(rec, x, threshold=0.01, win_ms=7.0, **odd)
    InpaintingEngine.find_gaps(rec, x, threshold=0.01, kind="held", **odd)
    InpaintingEngine.find_gaps(rec, x, threshold=0.01, kind="level", **odd)
    InpaintingEngine.find_gaps(rec, x, threshold=1.15, kind="burst", win_ms=4.0, **odd)
    InpaintingEngine.find_gaps(rec, x, kind="invalid", **odd)
    assert rec.calls == [("quiet", (0.01, 110), {"channel": None}),
                         ("dead", ("held", 0.01, 0.0, 0.0, 110), {"channel": None, "return_threshold": True}),
                         ("level", (), dict(half=22, threshold=0.01, rel_threshold=0.0, min_len=110, channel=None, return_threshold=True)),
                         ("burst", (), dict(half=44, threshold=1.15, rel_threshold=0.0, min_len=110, channel=None, return_threshold=True)),
                         ("invalid", (), dict(ceiling=float("inf"), min_len=110, channel=None))]


def test_conceal_routes_hand_the_new_keywords_to_kind_impulse_alone():
    calls = []

    def find_gaps(*a, **kw):
        calls.append(kw)
        return {"gaps": [], "skipped": [], "runs": None, "threshold": 0.5}

    patched = lambda *a, **kw: {"patched": torch.zeros(4)}
    eng = types.SimpleNamespace(device=torch.device("cpu"), recording_frames=lambda *a: (100, 100), find_gaps=find_gaps, patch_file=patched,
                                patch_recording=patched, _impulse_keywords=InpaintingEngine._impulse_keywords)
    x = torch.zeros(48000)
    base = {"kind": "impulse", "rel_threshold": 0.0, "held_tol": 0.0, "impulse_order": 16, "impulse_guard": 4, "impulse_pad": 2, "impulse_ratio": 10.0}
    InpaintingEngine.conceal_file(eng, x, 48000, kind="impulse", min_ms=0)
    assert calls[-1] == {"channel": None, **base}                       # win_ms not given: find_gaps puts 23 ms there
    InpaintingEngine.conceal_file(eng, x, 48000, kind="impulse", min_ms=0, win_ms=10.0, impulse_order=8, impulse_guard=8, impulse_pad=3, impulse_ratio=8.0)
    assert calls[-1] == {"channel": None, **base, "win_ms": 10.0, "impulse_order": 8, "impulse_guard": 8, "impulse_pad": 3, "impulse_ratio": 8.0}
    InpaintingEngine.conceal_file(eng, x, 48000, kind="impulse", min_ms=0, win_ms=2.0)
    assert calls[-1] == {"channel": None, **base, "win_ms": 2.0}        # 2.0 given is 2.0
    InpaintingEngine.conceal_recording(eng, x[:22050], kind="impulse", min_ms=0, win_ms=6.0, impulse_ratio=12.0)
    assert calls[-1] == {**base, "win_ms": 6.0, "impulse_ratio": 12.0}
    # the calls of before, whatever the new keywords say
    odd = dict(impulse_order=3, impulse_guard=1, impulse_pad=9, impulse_ratio=77.0)
    InpaintingEngine.conceal_file(eng, x, 48000, 0.25, kind="any", win_ms=3.0, **odd)
    assert calls[-1] == {"channel": None, "kind": "any", "rel_threshold": 0.0, "held_tol": 0.0}
    InpaintingEngine.conceal_file(eng, x, 48000, 0.25, kind="level", **odd)
    assert calls[-1] == {"channel": None, "kind": "level", "rel_threshold": 0.0, "held_tol": 0.0, "win_ms": 2.0}
    InpaintingEngine.conceal_file(eng, x, 48000, 1.15, kind="burst", win_ms=4.0, **odd)
    assert calls[-1] == {"channel": None, "kind": "burst", "rel_threshold": 0.0, "held_tol": 0.0, "win_ms": 4.0}
    InpaintingEngine.conceal_recording(eng, x[:22050], win_ms=1.0, **odd)
    assert calls[-1] == {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0}
    for fn in (InpaintingEngine.find_gaps, InpaintingEngine.conceal_file, InpaintingEngine.conceal_recording):
        p = inspect.signature(fn).parameters
        assert (p["impulse_order"].default, p["impulse_guard"].default, p["impulse_pad"].default, p["impulse_ratio"].default, p["win_ms"].default) == (16, 4, 2, 10.0, 2.0)
    p = inspect.signature(InpaintingEngine.find_impulse_runs).parameters
    assert [(k, v.default) for k, v in p.items()][2:] == [("win", None), ("half", None), ("order", 16), ("guard", 4), ("pad", 2), ("ratio", 10.0), ("threshold", 0.0),
                                                           ("rel_threshold", 0.0), ("min_len", 1), ("max_runs", 65536), ("channel", None), ("return_threshold", False)]
    assert [(k, v.default) for k, v in inspect.signature(InpaintingEngine.impulse_residual).parameters.items()][2:] == [("order", 16), ("channel", None)]


def test_find_impulse_runs_checks_its_arguments_before_the_device():
    eng = types.SimpleNamespace()
    for kw, msg in ((dict(), "win = its odd length"), (dict(win=5, half=2), "not both"), (dict(win=4), "win = 4: an odd number"),
                    (dict(half=4), r"half = 4 samples is under guard \+ 1 = 5: no sample would be left to compare with: widen the window or lower guard"),
                    (dict(half=1023), r"half \+ pad = 1025 samples, above 1024"), (dict(win=2051), r"half \+ pad = 1027 samples, above 1024"), (dict(half=1.5), "half = 1.5: a whole number of samples"),
                    (dict(half=64, order=1), "order = 1, outside 2 .. 32"), (dict(half=64, guard=65), "guard = 65 samples"), (dict(half=64, pad=17), "pad = 17 samples"),
                    (dict(half=64, ratio=0.99), r"ratio = 0.99 is NaN or outside \[1, 1e6\]"), (dict(half=64, rel_threshold=4.0001), r"rel_threshold = 4.0001 is NaN or outside \[0, 4\]")):
        with pytest.raises(ValueError, match="find_impulse_runs: .*" + msg):
            InpaintingEngine.find_impulse_runs(eng, np.zeros(8, np.float32), **kw)
    with pytest.raises(ValueError, match="impulse_residual: order = 33, outside 2 .. 32"):
        InpaintingEngine.impulse_residual(eng, np.zeros(8, np.float32), order=33)


# ------------------------------------------------------------------------------------------------------------ PCM scaling
def test_the_threshold_is_scaled_for_a_pcm_file_and_the_ratio_test_is_not(tmp_path, capsys):
    imp = types.SimpleNamespace(detect_dead={"kind": "impulse", "rel_threshold": 0.0, "held_tol": 0.0}, detect_level={"win_ms": 23.0},
                                detect_impulse={"ratio": 12.0, "order": 24, "guard": 6, "pad": 3})
    assert P.level_keywords(imp) == {"win_ms": 23.0}
    assert P.impulse_keywords(imp) == {"impulse_order": 24, "impulse_guard": 6, "impulse_pad": 3, "impulse_ratio": 12.0}
    other = types.SimpleNamespace(detect_dead={"kind": "burst", "rel_threshold": 0.0, "held_tol": 0.0}, detect_level={"win_ms": 4.0})
    assert P.impulse_keywords(other) == {} and P.impulse_keywords(types.SimpleNamespace()) == {}
    from scipy.io import wavfile
    calls = []

    def find_gaps(x, sr, thr, *a, **kw):
        calls.append((x.dtype, tuple(x.shape), thr, kw))
        return {"gaps": [(10, 3)], "skipped": [], "runs": None, "threshold": thr}

    engine = types.SimpleNamespace(recording_frames=lambda n22, clip: (100, 100), find_gaps=find_gaps)
    pcm = (np.arange(22050) % 200 - 100).astype(np.int16)
    want_kw = {"kind": "impulse", "rel_threshold": 0.0, "held_tol": 0.0, "win_ms": 23.0, "impulse_order": 24, "impulse_guard": 6, "impulse_pad": 3, "impulse_ratio": 12.0}
    record = {"win_ms": 23.0, "ratio": 12.0, "order": 24, "guard": 6, "pad": 3}
    for name, data, T, unit in (("pcm.wav", pcm, 0.25 * 32768, "int16 steps"), ("f32.wav", (pcm / 32768.0).astype(np.float32), 0.25, "full scale")):
        wavfile.write(tmp_path / name, 22050, data)
        cfg = types.SimpleNamespace(wave_path=str(tmp_path / name), detect={"threshold": 0.25, "min_ms": 0.0, "max_ms": 400.0, "pad_frames": 0},
                                    detect_dead=imp.detect_dead, detect_level=imp.detect_level, detect_impulse=imp.detect_impulse)
        assert P._detect_gaps(cfg, engine, data.astype(np.float32), 22050, 22050, 110, 200, 50, str(tmp_path)) == [(10, 3)]
        assert json.loads((tmp_path / "gaps.json").read_text()) == {"gaps": [[10, 3]], "skipped": [], "kind": "impulse", "T": T, **record}
        assert f"Detection kind = impulse, effective threshold T = {T} ({unit}), window win_ms = 23.0, ratio = 12.0, order = 24, guard = 6, pad = 3" in capsys.readouterr().out
    assert calls[0] == (np.int16, (22050,), 0.25 * 32768, want_kw) and calls[1] == (np.float32, (22050,), 0.25, want_kw)
    x24 = np.zeros((22050, 3), np.uint8)
    P._detect_gaps(cfg, engine, pcm.astype(np.float32), 22050, 22050, 110, 200, 50, str(tmp_path), x24=x24)
    assert calls[-1] == (np.uint8, (22050, 3), 0.25 * 8388608, want_kw)
    assert json.loads((tmp_path / "gaps.json").read_text()) == {"gaps": [[10, 3]], "skipped": [], "kind": "impulse", "T": 0.25 * 8388608, "unit": "24-bit steps", **record}
