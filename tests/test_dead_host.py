"""Held-sample and peak-relative dropouts, the parts that need no GPU: the declaration and its binding, the three new
keys of `detect:` in predict.yaml and their refusals, the routing of find_gaps between the two detectors, and the int16 scaling of
held_tol on the way from predict.yaml to the engine."""
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
    m = re.search(r"^int si_dead_runs\((.*?)\);", hdr, re.S | re.M)
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["si_ctx* ctx", "const void* x", "int is_pcm16", "int n", "int channels", "int channel", "int kind", "float threshold",
                    "float rel_threshold", "float held_tol", "int min_len", "int32_t* runs", "int max_runs", "int32_t* n_runs",
                    "float* threshold_out", "si_stream_t stream"]
    quiet = re.search(r"^int si_quiet_runs_ch\((.*?)\);", hdr, re.S | re.M).group(1).replace("\n", " ")
    assert [a for a in args if a not in ("int kind", "float rel_threshold", "float held_tol", "float* threshold_out")] == [a.strip() for a in quiet.split(",")]
    assert int(re.search(r"#define SI_DEAD_QUIET (\d+)\b", hdr).group(1)) == native.DEAD_QUIET == 1
    assert int(re.search(r"#define SI_DEAD_HELD (\d+)\b", hdr).group(1)) == native.DEAD_HELD == 2
    assert InpaintingEngine.DEAD_KINDS == {"quiet": 1, "held": 2, "any": 3}
    # the comment states the predicate, and where the reference stands
    doc = hdr[hdr.index("Held-sample and peak-relative dropouts"):m.start()]
    for phrase in ("The reference has no detection", "I_ea/predict.py:85-90", "max(threshold, fl32(rel_threshold * peak))", "link(i) or link(i + 1)",
                   "inf - inf", "65535", "never the adjacent elements", "EVERY channel's element is dead", "kind outside 1 .. 3",
                   "rel_threshold NaN or", "held_tol negative or NaN"):
        assert phrase in doc, phrase
    assert re.search(r"si_dead_runs\s+<- nothing the reference computes", hdr)
    assert "si_dead_runs" in native.EXPORTS and len(set(native.EXPORTS)) == len(native.EXPORTS)
    assert callable(native.NativeContext.dead_runs)
    api = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "api.hip")).read()
    assert re.search(r"^int si_dead_runs\(", api, re.M)
    if os.path.exists(native.LIB_PATH):
        lib = native.load_library()
        assert lib.si_version() == 3 and len(lib.si_dead_runs.argtypes) == len(args)


# ------------------------------------------------------------------------------------------------------------ predict.yaml
def _yaml(tmp_path, extra, drop=("mask",)):
    data = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "iea_predict.yaml")))
    for key in drop:
        data.pop(key, None)
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_detect_keys(tmp_path):
    defaults = {"threshold": 0.0, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0}
    plain = {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0}
    assert load_predict_config(_yaml(tmp_path, "long: {}\n")).detect_dead is None
    cfg = load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {}\n"))
    assert cfg.detect == defaults and cfg.detect_dead == plain                       # the four keys of before stay what they were
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file}\ndetect: {kind: held, held_tol: 0.001, min_ms: 2, channels: joint}\n"))
    assert cfg.detect == {**defaults, "min_ms": 2.0} and cfg.detect_dead == {**plain, "kind": "held", "held_tol": 0.001} and cfg.detect_channels == "joint"
    cfg = load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: any, rel_threshold: 1.0e-3, threshold: 0.0001}\n"))
    assert cfg.detect_dead == {"kind": "any", "rel_threshold": 1e-3, "held_tol": 0.0} and cfg.detect["threshold"] == 1e-4
    assert load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {rel_threshold: 1}\n")).detect_dead["rel_threshold"] == 1.0
    with pytest.raises(ValueError, match="detect.kind = 'silence': quiet .* held .* or any"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: silence}\n"))
    with pytest.raises(ValueError, match="detect.rel_threshold = -0.5 is negative"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {rel_threshold: -0.5}\n"))
    with pytest.raises(ValueError, match="detect.rel_threshold = 1.5 is a fraction of the file's peak, at most 1"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {rel_threshold: 1.5}\n"))
    with pytest.raises(ValueError, match="detect.rel_threshold = nan is negative"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {rel_threshold: .nan}\n"))
    with pytest.raises(ValueError, match="detect.held_tol = -1.0 is negative"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {held_tol: -1}\n"))
    with pytest.raises(ValueError, match=r"unknown key `kinds` in `detect:` \(it takes threshold, min_ms, max_ms, pad_frames, channels, kind, rel_threshold, held_tol\)"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kinds: held}\n"))


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


def test_find_gaps_routes_between_the_two_detectors():
    x = torch.zeros(22050)
    rec = _Recorder()
    out = InpaintingEngine.find_gaps(rec, x, threshold=0.01, min_ms=5.0)
    assert rec.calls == [("quiet", (0.01, 110), {"channel": None})]                  # the defaults: find_quiet_runs, called as it was
    assert sorted(out) == ["gaps", "runs", "skipped"] and out["gaps"] == [(10, 3)]
    for kw in (dict(kind="quiet", rel_threshold=0.0, held_tol=0.0), dict(kind="quiet")):
        rec.calls.clear()
        InpaintingEngine.find_gaps(rec, x, threshold=0.01, **kw)
        assert [c[0] for c in rec.calls] == ["quiet"]
    for kw in (dict(kind="held"), dict(kind="any"), dict(rel_threshold=1e-3), dict(held_tol=1e-4), dict(kind="held", held_tol=2.0, rel_threshold=0.5)):
        rec.calls.clear()
        out = InpaintingEngine.find_gaps(rec, x, threshold=0.01, channel=None, **kw)
        full = {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0, **kw}
        assert rec.calls == [("dead", (full["kind"], 0.01, full["rel_threshold"], full["held_tol"], 110), {"channel": None, "return_threshold": True})]
        assert out["threshold"] == 0.125 and out["gaps"] == [(10, 3)]


# ------------------------------------------------------------------------------------------------------------ int16 scaling
def test_held_tol_is_scaled_for_an_int16_file_and_rel_threshold_is_not(tmp_path, capsys):
    dead = {"kind": "any", "rel_threshold": 1e-3, "held_tol": 2.0 / 32768}
    assert P.dead_keywords(dead, 32768.0) == {"kind": "any", "rel_threshold": 1e-3, "held_tol": 2.0}
    assert P.dead_keywords(dead, 1.0) == dead and P.dead_keywords(None, 32768.0) == {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0}
    # through _detect_gaps, on an int16 file and on a float one
    from scipy.io import wavfile
    calls = []

    def find_gaps(x, sr, thr, *a, **kw):
        calls.append((x.dtype, thr, kw))
        return {"gaps": [(10, 3)], "skipped": [], "runs": None, **({"threshold": 6.5} if kw["kind"] != "quiet" or kw["rel_threshold"] or kw["held_tol"] else {})}

    engine = types.SimpleNamespace(recording_frames=lambda n22, clip: (100, 100), find_gaps=find_gaps)
    pcm = (np.arange(22050) % 200 - 100).astype(np.int16)
    for name, data in (("pcm.wav", pcm), ("f32.wav", (pcm / 32768.0).astype(np.float32))):
        wavfile.write(tmp_path / name, 22050, data)
        cfg = types.SimpleNamespace(wave_path=str(tmp_path / name), detect={"threshold": 3.0 / 32768, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0},
                                    detect_dead=dead)
        assert P._detect_gaps(cfg, engine, data.astype(np.float32), 22050, 22050, 110, 200, 50, str(tmp_path)) == [(10, 3)]
        assert json.loads((tmp_path / "gaps.json").read_text()) == {"gaps": [[10, 3]], "skipped": [], "kind": "any", "T": 6.5}
    assert calls[0] == (np.int16, 3.0, {"kind": "any", "rel_threshold": 1e-3, "held_tol": 2.0})
    assert calls[1] == (np.float32, 3.0 / 32768, {"kind": "any", "rel_threshold": 1e-3, "held_tol": 2.0 / 32768})
    printed = capsys.readouterr().out
    assert "Detection kind = any, effective threshold T = 6.5 (int16 steps)" in printed and "T = 6.5 (full scale)" in printed
    # at the defaults gaps.json is what it was
    cfg.detect_dead = {"kind": "quiet", "rel_threshold": 0.0, "held_tol": 0.0}
    P._detect_gaps(cfg, engine, data.astype(np.float32), 22050, 22050, 110, 200, 50, str(tmp_path))
    assert json.loads((tmp_path / "gaps.json").read_text()) == {"gaps": [[10, 3]], "skipped": []}
