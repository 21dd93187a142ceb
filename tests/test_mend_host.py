"""Short runs mended by least-squares AR interpolation, the parts that need no GPU: the declaration of si_mend_runs, its
binding and export, the profile name of its launcher, the `detect: {mend_ms, mend_order, mend_context}` keys of predict.yaml with their
defaults and refusals, the routing of conceal_file with a stub engine -- mended rows leave the gap list, a joint run needs every channel,
mend_ms = 0 calls nothing new -- and the text of every refusal."""
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
from tests import mend_ref as M
from tests import poison

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_inpainting_amd", "csrc")


# ------------------------------------------------------------------------------------------------------------ ABI
def test_the_entry_point_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "si_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    args = [a.strip() for a in re.search(r"^int si_mend_runs\((.*?)\);", code, flags=re.S | re.M).group(1).replace("\n", " ").split(",")]
    assert args == ["si_ctx* ctx", "void* x", "int is_pcm16", "int n", "int channels", "int channel", "const int32_t* runs", "int n_runs", "int max_len",
                    "int order", "int context", "int32_t* status", "si_stream_t stream"]
    assert re.search(r"#define SI_ABI_VERSION 3\b", hdr) and re.search(r"si_mend_runs\s+<- nothing the reference computes", hdr)
    for name, value in (("MAX_LEN", 64), ("MAX_ORDER", 32), ("MAX_CONTEXT", 1024), ("MAX_RUNS", 65536), ("LONG", 0), ("AR", 1), ("LINE", 2), ("EDGE", 3),
                        ("NEAR", 4), ("NONFINITE", 5), ("BADROW", 6)):
        assert re.search(rf"#define SI_MEND_{name} {value}\b", hdr), name
        assert getattr(native, f"MEND_{name}") == value and (name.startswith("MAX") or (getattr(M, name) == value and native.MEND_STATUS[value] == name))
    doc = hdr[hdr.index("Short damaged runs mended in place"):hdr.index("#define SI_MEND_MAX_LEN")]
    for phrase in ("DESIGN.md 4.31", "IN PLACE", "sorted and disjoint", "r[0] *= 1 + 1e-9", "Levinson-Durbin", "a pivot <= 0: LINE", "ties to even",
                   "nothing before the whole solve has succeeded", "a row alone gives the bytes of the same row inside a table", "No atomics",
                   'profiled in the family "patch_rate"', "SI_EINVAL before any launch", "n_runs = 0 launches\n * nothing"):
        assert phrase in doc, phrase
    assert "si_mend_runs" in native.EXPORTS and len(set(native.EXPORTS)) == len(native.EXPORTS)
    assert callable(native.NativeContext.mend_runs) and callable(InpaintingEngine.mend_runs)
    api = open(os.path.join(CSRC, "api.hip")).read()
    body = api[api.index("int si_mend_runs("):api.index("#undef SI_FAIL_FN")]
    assert body.index("if (n_runs == 0) return SI_OK;") < body.index("si_launch_mend_runs(") and body.count("SI_FAIL_FN(") == 8
    assert "mend_kernels.hip" in open(os.path.join(CSRC, "Makefile")).read()
    kern = open(os.path.join(CSRC, "mend_kernels.hip")).read()
    assert "atomic" not in kern.replace("No atomics", "") and "WRITE SET" in kern and "READ SET" in kern
    p = inspect.signature(InpaintingEngine.mend_runs).parameters
    assert [(k, v.default) for k, v in p.items()][3:] == [("max_len", 64), ("order", 32), ("context", 512), ("channel", None), ("inplace", False)]
    if os.path.exists(native.LIB_PATH):
        lib = native.load_library()
        assert lib.si_version() == 3 and len(lib.si_mend_runs.argtypes) == len(args)


def test_the_launcher_uses_a_profile_name_of_the_closed_lists():
    """The launch has no scratch and writes into the caller's copy of the file: it runs in patch_rate's family, which tests/poison.py lists
    among the families without scratch."""
    src = open(os.path.join(CSRC, "mend_kernels.hip")).read()
    names = re.findall(r'si_prof_begin\(ctx, "(\w+)"', src)
    assert names == ["patch_rate"] and "patch_rate" in poison.NO_SCRATCH_FAMILIES and "patch_rate" not in poison.SCRATCH_FAMILIES


# ------------------------------------------------------------------------------------------------------------ predict.yaml
def _yaml(tmp_path, extra, drop=("mask",)):
    data = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "iea_predict.yaml")))
    for key in drop:
        data.pop(key, None)
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_mend_keys(tmp_path):
    long = "long: {rate: file, feed: contexts}\n"
    cfg = load_predict_config(_yaml(tmp_path, long + "detect: {kind: invalid, mend_ms: 1.0}\n"))
    assert cfg.detect_mend == {"mend_ms": 1.0, "mend_order": 32, "mend_context": 512} and cfg.detect["min_ms"] == 0.0
    cfg = load_predict_config(_yaml(tmp_path, long + "detect: {min_ms: 0.1, mend_ms: 0.5, mend_order: 8, mend_context: 64}\n"))
    assert cfg.detect_mend == {"mend_ms": 0.5, "mend_order": 8, "mend_context": 64}
    assert cfg.detect == {"threshold": 0.0, "min_ms": 0.1, "max_ms": 400.0, "pad_frames": 0}        # the mapping of before: no new key in it
    # absent keys, and mend_ms: 0, leave the parse result as it is
    plain = load_predict_config(_yaml(tmp_path, long + "detect: {kind: invalid}\n"))
    zero = load_predict_config(_yaml(tmp_path, long + "detect: {kind: invalid, mend_ms: 0}\n"))
    assert plain.detect_mend is None and zero.detect_mend is None and plain.detect == zero.detect and plain.detect_dead == zero.detect_dead
    assert load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {}\n")).detect_mend is None
    assert P.mend_keywords(plain) == {} and P.mend_keywords(types.SimpleNamespace(detect=None)) == {} and P.mend_keywords(types.SimpleNamespace(detect={})) == {}
    assert P.mend_keywords(cfg) == {"mend_ms": 0.5, "mend_order": 8, "mend_context": 64}
    for rate, key in (("{}", "mend_ms"), ("{rate: 22050}", "mend_ms")):
        with pytest.raises(ValueError, match=rf"detect.{key} needs `long: \{{rate: file\}}`"):
            load_predict_config(_yaml(tmp_path, f"long: {rate}\ndetect: {{kind: invalid, mend_ms: 1.0}}\n"))
    with pytest.raises(ValueError, match=r"detect.mend_order needs `long: \{rate: file\}`"):
        load_predict_config(_yaml(tmp_path, "long: {}\ndetect: {kind: invalid, mend_order: 8}\n"))
    with pytest.raises(ValueError, match=r"detect.mend_context without detect.mend_ms"):
        load_predict_config(_yaml(tmp_path, long + "detect: {kind: invalid, mend_context: 64}\n"))
    with pytest.raises(ValueError, match=r"detect.mend_ms = -1.0 is negative or not finite"):
        load_predict_config(_yaml(tmp_path, long + "detect: {kind: invalid, mend_ms: -1}\n"))
    with pytest.raises(ValueError, match=r"detect.mend_order = 33, outside 2 .. 32"):
        load_predict_config(_yaml(tmp_path, long + "detect: {kind: invalid, mend_ms: 1, mend_order: 33}\n"))
    with pytest.raises(ValueError, match=r"detect.mend_context = 100 samples, outside 4 \* mend_order = 128 .. 1024"):
        load_predict_config(_yaml(tmp_path, long + "detect: {kind: invalid, mend_ms: 1, mend_context: 100}\n"))
    with pytest.raises(ValueError, match=r"detect.min_ms = 5.0 is not under detect.mend_ms = 1.0"):
        load_predict_config(_yaml(tmp_path, long + "detect: {mend_ms: 1.0}\n"))                       # min_ms keeps its default of 5 off kind: invalid
    with pytest.raises(ValueError, match=r"unknown key `mend` in `detect:`"):
        load_predict_config(_yaml(tmp_path, long + "detect: {kind: invalid, mend: 1}\n"))


# ------------------------------------------------------------------------------------------------------------ routing
class _Stub:
    """Stands in for an engine under conceal_file: find_gaps returns `runs`, mend_runs fills the rows `fills[channel]` names."""
    device = torch.device("cpu")
    _mend_limits = staticmethod(InpaintingEngine._mend_limits)
    _conceal_mended = InpaintingEngine._conceal_mended

    def __init__(self, runs, fills):
        self.runs, self.fills, self.calls = torch.tensor(runs, dtype=torch.int32).reshape(-1, 2), fills, []

    def recording_frames(self, *a):
        return 300, 300

    def find_gaps(self, x, sr, *a, **kw):
        self.calls.append(("find_gaps", kw["channel"]))
        return {"gaps": [(-1, -1)], "skipped": [], "runs": self.runs, "threshold": float("inf")}

    def mend_runs(self, y, runs, max_len, order, context, channel=None, inplace=False):
        self.calls.append(("mend_runs", max_len, order, context, channel, inplace))
        fill = self.fills[channel]
        return y, torch.tensor([fill.get(i, native.MEND_LONG if int(runs[i, 1]) > max_len else native.MEND_NEAR) for i in range(runs.shape[0])], dtype=torch.int32)

    def patch_file(self, y, sr, gaps=None, **kw):
        self.calls.append(("patch_file", gaps, kw))
        return {"patched": y}


RUNS = [(960 * 10 + 5, 1), (960 * 20, 3), (960 * 30, 9600), (960 * 60 + 7, 48), (960 * 70, 49)]
BASE = dict(fade_ms=5.0, clip_frames=200, min_context=50, batch=32, return_windows=False, feed="contexts", ceiling=float("inf"))


def test_mended_rows_leave_the_gap_list():
    eng = _Stub(RUNS, {None: {0: native.MEND_AR, 1: native.MEND_LINE, 3: native.MEND_EDGE}})
    x = torch.zeros(48000 * 6)
    out = InpaintingEngine.conceal_file(eng, x, 48000, min_ms=0, kind="invalid", feed="contexts", mend_ms=1.0)
    assert eng.calls[0] == ("find_gaps", None) and eng.calls[1] == ("mend_runs", 48, 32, 512, None, True)
    assert eng.calls[2] == ("patch_file", [(30, 10), (60, 1), (70, 1)], BASE) and len(eng.calls) == 3
    assert out["gaps"] == [(30, 10), (60, 1), (70, 1)] and out["skipped"] == [] and out["threshold"] == float("inf")
    assert out["mended"] == [(RUNS[0][0], 1, native.MEND_AR), (RUNS[1][0], 3, native.MEND_LINE), (RUNS[3][0], 48, native.MEND_EDGE)]      # len <= max_len only
    assert out["patched"].data_ptr() != x.data_ptr()                   # the mending ran on a copy
    eng = _Stub(RUNS, {None: {}})
    InpaintingEngine.conceal_file(eng, x, 24000, min_ms=0, kind="invalid", feed="contexts", mend_ms=2.0, mend_order=8, mend_context=64)
    assert eng.calls[1] == ("mend_runs", 48, 8, 64, None, True)                                      # max_len = round(mend_ms sr / 1000)
    eng = _Stub(np.zeros((0, 2)), {None: {}})                          # nothing found: nothing mended, patch_file with no gaps
    out = InpaintingEngine.conceal_file(eng, x, 48000, min_ms=0, kind="invalid", feed="contexts", mend_ms=1.0)
    assert [c[0] for c in eng.calls] == ["find_gaps", "patch_file"] and out["mended"] == [] and out["gaps"] == []


def test_each_channel_mends_its_own_runs_and_joint_needs_every_channel():
    x = torch.zeros(48000 * 6, 2)
    eng = _Stub(RUNS[:2], {0: {0: native.MEND_AR}, 1: {0: native.MEND_AR, 1: native.MEND_AR}})
    out = InpaintingEngine.conceal_file(eng, x, 48000, min_ms=0, kind="invalid", feed="contexts", detect="each", mend_ms=1.0)
    assert [c[:2] for c in eng.calls[:4]] == [("find_gaps", 0), ("find_gaps", 1), ("mend_runs", 48), ("mend_runs", 48)] and [c[4] for c in eng.calls[2:4]] == [0, 1]
    assert eng.calls[4][0] == "patch_file" and eng.calls[4][1] is None and eng.calls[4][2] == {**BASE, "channel_gaps": [[(20, 1)], []]}
    assert out["gaps"] == [[(20, 1)], []] and out["skipped"] == [[], []] and out["threshold"] == [float("inf")] * 2
    assert out["mended"] == [[(RUNS[0][0], 1, native.MEND_AR), (RUNS[1][0], 3, native.MEND_NEAR)], [(RUNS[0][0], 1, native.MEND_AR), (RUNS[1][0], 3, native.MEND_AR)]]
    eng = _Stub(RUNS[:2], {0: {0: native.MEND_AR, 1: native.MEND_NONFINITE}, 1: {0: native.MEND_LINE, 1: native.MEND_AR}})
    out = InpaintingEngine.conceal_file(eng, x, 48000, min_ms=0, kind="invalid", feed="contexts", detect="joint", mend_ms=1.0)
    assert [c[:2] for c in eng.calls[:3]] == [("find_gaps", -1), ("mend_runs", 48), ("mend_runs", 48)] and [c[4] for c in eng.calls[1:3]] == [0, 1]
    assert eng.calls[3] == ("patch_file", [(20, 1)], BASE)             # row 1 stays a gap: channel 0 did not fill it
    assert out["mended"] == [(RUNS[0][0], 1, native.MEND_LINE), (RUNS[1][0], 3, native.MEND_NONFINITE)] and out["gaps"] == [(20, 1)]


def test_mend_ms_zero_calls_nothing_new():
    seen = []
    eng = types.SimpleNamespace(device=torch.device("cpu"), recording_frames=lambda *a: (100, 100),
                                find_gaps=lambda *a, **kw: seen.append(("find_gaps", a[1:], kw)) or {"gaps": [(3, 1)], "skipped": [], "runs": None},
                                patch_file=lambda *a, **kw: seen.append(("patch_file", a[1:], kw)) or {"patched": torch.zeros(4)})
    x = torch.zeros(48000)
    a = InpaintingEngine.conceal_file(eng, x, 48000, 0.01)
    first, seen[:] = list(seen), []
    b = InpaintingEngine.conceal_file(eng, x, 48000, 0.01, mend_ms=0.0, mend_order=8, mend_context=64)
    assert seen == first and sorted(a) == sorted(b) == ["gaps", "patched", "skipped"]               # no mend_runs attribute was touched, no `mended`
    p = inspect.signature(InpaintingEngine.conceal_file).parameters
    assert list(p)[-3:] == ["mend_ms", "mend_order", "mend_context"] and [p[k].default for k in list(p)[-3:]] == [0.0, 32, 512]
    for fn in (InpaintingEngine.conceal_recording, InpaintingEngine.patch_file, InpaintingEngine.patch_recording, InpaintingEngine.find_gaps):
        assert not [k for k in inspect.signature(fn).parameters if k.startswith("mend")], fn      # out of scope, unchanged


# ------------------------------------------------------------------------------------------------------------ refusals
def test_the_text_of_every_refusal():
    eng = _Stub(RUNS, {None: {}})
    x = torch.zeros(48000)
    call = lambda **kw: InpaintingEngine.conceal_file(eng, x, 48000, **{"min_ms": 0, "kind": "invalid", "feed": "contexts", **kw})
    with pytest.raises(ValueError, match=r"conceal_file: mend_ms = 1.5 at 48000 Hz is max_len = 72 samples, at most 64: lower mend_ms to 1.333 or less; "
                                         r"longer runs stay with the inpainter"):
        call(mend_ms=1.5)
    with pytest.raises(ValueError, match=r"conceal_file: min_ms = 1.0 is not under mend_ms = 1.0: no run short enough to mend would be reported; lower min_ms"):
        call(mend_ms=1.0, min_ms=1.0)
    with pytest.raises(ValueError, match=r"conceal_file: min_ms = 5.0 is not under mend_ms = 1.0"):
        InpaintingEngine.conceal_file(eng, x, 48000, mend_ms=1.0)
    with pytest.raises(ValueError, match=r"conceal_file: mend_ms = -1.0 is negative or NaN"):
        call(mend_ms=-1.0)
    with pytest.raises(ValueError, match=r"conceal_file: mend_ms = 0.001 at 48000 Hz is less than one sample: raise it to 0.021 or more, or pass 0"):
        call(mend_ms=0.001)
    with pytest.raises(ValueError, match=r"conceal_file: order = 40, outside 2 .. 32"):
        call(mend_ms=1.0, mend_order=40)
    with pytest.raises(ValueError, match=r"conceal_file: context = 100 samples, outside 4 \* order = 128 .. 1024: raise context or lower order"):
        call(mend_ms=1.0, mend_context=100)
    assert eng.calls == []                                             # each before any detection
    bare = InpaintingEngine.__new__(InpaintingEngine)
    bare.device = torch.device("cpu")
    f = np.zeros(4096, np.float32)
    with pytest.raises(ValueError, match=r"mend_runs: max_len = 65 samples, at most 64: .* leave longer runs to the inpainter \(lower max_len / mend_ms\)"):
        bare.mend_runs(f, [(100, 2)], max_len=65)
    with pytest.raises(ValueError, match=r"mend_runs: max_len = 0 samples, at least 1"):
        bare.mend_runs(f, [(100, 2)], max_len=0)
    with pytest.raises(ValueError, match=r"mend_runs: order = 1, outside 2 .. 32"):
        bare.mend_runs(f, [(100, 2)], order=1)
    with pytest.raises(ValueError, match=r"mend_runs: context = 1025 samples, outside 4 \* order = 128 .. 1024"):
        bare.mend_runs(f, [(100, 2)], context=1025)
    with pytest.raises(ValueError, match=r"mend_runs: an \(n, 2\) recording needs channel = an index"):
        bare.mend_runs(np.zeros((4096, 2), np.float32), [(100, 2)])
    with pytest.raises(ValueError, match=r"mend_runs: an \(n, 2\) recording needs channel = an index"):
        bare.mend_runs(np.zeros((4096, 2), np.float32), [(100, 2)], channel=-1)
    with pytest.raises(ValueError, match=r"mend_runs: channel = 1 of a one-channel recording"):
        bare.mend_runs(f, [(100, 2)], channel=1)
    with pytest.raises(ValueError, match=r"mend_runs: a uint8 input is packed 24-bit PCM"):
        bare.mend_runs(np.zeros(4096, np.uint8), [(100, 2)])
    with pytest.raises(ValueError, match=r"mend_runs: inplace = True needs a contiguous device tensor"):
        bare.mend_runs(f, [(100, 2)], inplace=True)
    for rows, text in (([(100, 2), (101, 3)], r"row 1 = \(start 101, len 3\) starts before row 0 ends at 102: rows are sorted and disjoint"),
                       ([(200, 2), (100, 3)], r"row 1 = \(start 100, len 3\) starts before row 0 ends at 202"),
                       ([(100, 0)], r"row 0 = \(start 100, len 0\) is empty or outside the file's 4096 samples"),
                       ([(-1, 2)], r"row 0 = \(start -1, len 2\) is empty or outside the file's 4096 samples"),
                       ([(10, 2), (4095, 2)], r"row 1 = \(start 4095, len 2\) is empty or outside the file's 4096 samples")):
        with pytest.raises(ValueError, match="mend_runs: " + text):
            bare.mend_runs(f, rows)
        with pytest.raises(ValueError):
            M.check_runs(rows, 4096)
    M.check_runs([(100, 2), (102, 3)], 4096)                           # touching rows are disjoint


# ------------------------------------------------------------------------------------------------------------ the CLI
def test_the_cli_routes_mend_ms_through_conceal_file_and_records_the_count(tmp_path, capsys):
    from scipy.io import wavfile
    x = (0.25 * np.sin(np.arange(48000) / 30.0)).astype(np.float32)
    x[24000] = np.nan
    wavfile.write(tmp_path / "f.wav", 48000, x)
    seen = []

    def conceal_file(xx, sr, thr, min_ms, max_ms, pad, **kw):
        seen.append((sr, thr, min_ms, max_ms, pad, kw))
        return {"patched": torch.from_numpy(np.nan_to_num(xx)), "labels": torch.zeros(1, dtype=torch.int64), "label_off": [0, 1], "gaps": [(30, 2)],
                "skipped": [(0, 1, "edge")], "threshold": float("inf"),
                "mended": [(3, 1, native.MEND_EDGE), (24000, 1, native.MEND_AR), (30000, 2, native.MEND_AR), (40000, 5, native.MEND_NEAR)]}

    engine = types.SimpleNamespace(conceal_file=conceal_file)          # neither find_gaps nor patch_file: the route is conceal_file alone
    mk = lambda mend: types.SimpleNamespace(wave_path=str(tmp_path / "f.wav"), long={"clip_s": 4.0, "context_s": 1.0, "batch": 32}, long_feed="contexts",
                                            long_clips16="resampled", long_pcm24="float32", patch_fade_ms=None, gaps=None,
                                            detect={"threshold": 0.0, "min_ms": 0.0, "max_ms": 400.0, "pad_frames": 0},
                                            detect_dead={"kind": "invalid", "rel_threshold": 0.0, "held_tol": 0.0}, detect_level={"win_ms": 2.0},
                                            detect_mend=mend)
    assert P._main_long_file(mk({"mend_ms": 1.0, "mend_order": 16, "mend_context": 256}), engine, str(tmp_path)) == 0
    assert seen[-1][:5] == (48000, 0.0, 0.0, 400.0, 0)
    assert seen[-1][5] == dict(fade_ms=5.0, clip_frames=200, min_context=50, batch=32, feed="contexts", kind="invalid", rel_threshold=0.0, held_tol=0.0,
                               mend_ms=1.0, mend_order=16, mend_context=256)
    assert json.loads((tmp_path / "gaps.json").read_text()) == {"gaps": [[30, 2]], "skipped": [[0, 1, "edge"]], "kind": "invalid", "ceiling": None,
                                                               "mended": {"EDGE": 1, "AR": 2, "NEAR": 1}}
    assert "Mended runs of at most 1.0 ms, by status: {'EDGE': 1, 'AR': 2, 'NEAR': 1}" in capsys.readouterr().out
    assert P.mended_report([]) == {}
    # without the keys the route is find_gaps + patch_file, as it was: this engine has neither
    with pytest.raises(AttributeError, match="recording_frames"):
        P._main_long_file(mk(None), engine, str(tmp_path))
