"""engine.conceal_file held to its own parts over every allowed pair of its keywords, with the tiny random model.

One parametrized test runs the covering set of tests/conceal_cases.py.  Per case:
    1  gaps, skipped, threshold and mended equal what the float64 references give for the case's file (detect_ref, channels_ref, dead_ref,
       level_ref, burst_ref, invalid_ref, impulse_ref, mend_ref, gaps.runs_to_gaps), exactly and per channel where the route returns them
       per channel; the mended samples meet tests/test_gpu_mend.py's comparator;
    2  the same input through the public pieces by hand -- find_gaps, mend_runs(inplace=True) on a clone, gaps.runs_to_gaps, patch_file --
       gives the same dictionary: the same keys, every tensor bit for bit, every list and number equal;
    3  outside the mended runs and the gaps' spans widened by the file-rate fade, `patched` holds the input's bits, NaN payloads included;
       `patched` has the input's dtype and shape and lies on the engine's device.
Beside the sweep: an (n, 1) file against its (n,) flattening and a host array against a device tensor return equal dictionaries; and one
forbidden call per constraint is refused before anything is launched."""
import time

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from tests import conceal_cases as CC
from tests import mend_ref as M
from tests import s24_ref as S
from tests import test_gpu_mend as TM
from tests.harness import build_engine

pytestmark = pytest.mark.gpu

IDS, CASES = CC.covering_set()
FILLED = (native.MEND_AR, native.MEND_LINE)
SUMMARY = {"cases": 0, "fp32": 0.0, "pcm_odd": 0, "mended_samples": 0, "t0": time.time(), "gpu_s": 0.0}


def _engine():
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    return build_engine(HubertArch.tiny(), VocoderArch.v1(), 100, "fp32", "fp32", key=("patch", "fp32"))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.int16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, where="out"):
    """a == b all the way down: tensors by dtype, shape, device kind and bits; dictionaries by their keys; lists by length."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and a.device.type == b.device.type, where
        assert torch.equal(_bits(a), _bits(b)), (where, int((_bits(a) != _bits(b)).sum()))
    elif isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), (where, sorted(a), sorted(b) if isinstance(b, dict) else b)
        for k in a:
            _same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), (where, a, b)
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, f"{where}[{i}]")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif hasattr(a, "__dict__"):                                        # a pass's RateTable: its counts, its host image and its device copy
        assert type(a) is type(b), (where, type(a), type(b))
        _same(vars(a), vars(b), where)
    else:
        assert a == b and type(a) is type(b), (where, a, b)


def _by_parts(eng, x, sr, kw):
    """conceal_file(x, sr, **kw) as its docstring composes it, from the public calls -> (the dictionary, the mended copy or None, the
    statuses mend_runs returned per mended channel)."""
    s24 = x.dtype == torch.uint8
    ch = x.shape[1] if x.dim() - int(s24) == 2 else 1
    many, each = ch >= 2, kw.get("detect", "each") == "each"
    flat = x if many else (x.reshape(-1, 3) if s24 else x.reshape(-1))
    n = flat.shape[0]
    clip, ctx = kw["clip_frames"], kw["min_context"]
    P, Q = G.rate_ratio(sr)
    n_rec, lim = eng.recording_frames(-(-n * P // Q), clip)
    max_ms = min(400.0, 20.0 * (clip - 2 * ctx)) if n_rec > clip else 400.0
    fade22 = -(-G.file_fade(5.0, sr) * P // Q)
    min_ms = kw.get("min_ms", 5.0)
    det = {k: kw[k] for k in ("kind", "rel_threshold", "win_ms") if k in kw}
    find = lambda c: eng.find_gaps(flat, sr, kw["threshold"], min_ms, max_ms, 0, None, fade22, n_rec, lim, channel=c, **det)
    pkw = dict(clip_frames=clip, min_context=ctx, batch=kw["batch"], feed=kw["feed"], clips16=kw["clips16"], return_windows=kw.get("return_windows", False))
    if kw["kind"] == "invalid":
        pkw["ceiling"] = G.invalid_ceiling(kw["threshold"])             # no other kind hands patch_file a ceiling
    channels = list(range(ch)) if (many and each) else [-1 if many else None]
    found = [find(c) for c in channels]
    extra, y, statuses = {}, None, []
    if "mend_ms" in kw:
        max_len = int(round(kw["mend_ms"] * sr / 1000.0))
        mf = 2 * max(-(-fade22 // 441), 1)                               # merge_frames None: find_gaps' documented default
        y = flat.to(eng.device).clone()
        gaps, skipped, mended = [], [], []
        for c, f in zip(channels, found):
            rows = [(int(s), int(l)) for s, l in f["runs"].tolist()]
            mend_in = list(range(ch)) if c == -1 else [c]               # joint: every channel, in channel order
            per = [eng.mend_runs(y, f["runs"], max_len, kw["mend_order"], kw["mend_context"], channel=m, inplace=True)[1].tolist() if rows else []
                   for m in mend_in]
            statuses += [(m, st) for m, st in zip(mend_in, per) if rows]       # a channel without runs has no reference to meet
            status = []
            for i in range(len(rows)):
                col = [st[i] for st in per]
                bad = [v for v in col if v not in FILLED]
                status.append(bad[0] if bad else native.MEND_LINE if native.MEND_LINE in col else native.MEND_AR)
            mended.append([(s, l, st) for (s, l), st in zip(rows, status) if l <= max_len])
            g, k = G.runs_to_gaps([r for r, st in zip(rows, status) if st not in FILLED], n, sr, n_rec, lim, 0, mf, max(int(max_ms // 20), 1))
            gaps.append(g)
            skipped.append(k)
        extra["mended"] = mended if (many and each) else mended[0]
        source = y.reshape(x.shape)
    else:
        gaps, skipped, source = [f["gaps"] for f in found], [f["skipped"] for f in found], x
    if many and each:
        out = eng.patch_file(source, sr, channel_gaps=gaps, **pkw)
        out["gaps"], out["skipped"] = gaps, skipped
        if "threshold" in found[0]:
            out["threshold"] = [f["threshold"] for f in found]
    else:
        out = eng.patch_file(source, sr, gaps[0], **pkw)
        out["gaps"], out["skipped"] = gaps[0], skipped[0]
        if "threshold" in found[0]:
            out["threshold"] = found[0]["threshold"]
    out.update(extra)
    return out, y, statuses


def _host(t, case):
    """A result tensor as a host array in the references' dtype and the file's layout."""
    a = t.cpu().numpy()
    return S.unpack(a).astype(M.S24) if case["stype"] == "s24" else a


def _raw(a):
    """(n, ch, bytes per sample) uint8 of a host file in the references' dtype."""
    n = a.shape[0]
    if a.dtype.type is M.S24:
        return S.pack(a).reshape(n, -1, 3)
    return np.ascontiguousarray(a).view(np.uint8).reshape(n, -1, a.itemsize)


def _check_case(eng, case):
    e = CC.expected(case)
    x, sr, kw = e["x"], case["sr"], e["kw"]
    xin = CC.as_input(x, case, eng.device)
    t0 = time.time()
    got = eng.conceal_file(xin, sr, **kw)
    parts, y, statuses = _by_parts(eng, xin, sr, kw)
    torch.cuda.synchronize()
    SUMMARY["gpu_s"] += time.time() - t0
    each = CC.detect_of(case) == "each"
    ch = CC.CHANNELS[case["layout"]]
    per = (lambda v: v) if each else (lambda v: [v] * ch)
    # ---- 1: against the references
    assert got["gaps"] == e["gaps"] and got["skipped"] == e["skipped"], (got["gaps"], e["gaps"], got["skipped"], e["skipped"])
    assert ("threshold" in got) == ("threshold" in e) and got.get("threshold") == e.get("threshold"), (got.get("threshold"), e.get("threshold"))
    assert ("mended" in got) == (case["mend"] == "on") and got.get("mended") == e.get("mended"), (got.get("mended"), e.get("mended"))
    patched = got["patched"]
    assert patched.dtype == xin.dtype and patched.shape == xin.shape and patched.device.type == eng.device.type
    ph, x2 = _host(patched, case).reshape(x.shape[0], ch), x.reshape(x.shape[0], ch)
    allowed = np.stack([CC.blend_set(x.shape[0], g, sr) for g in per(got["gaps"])], axis=1)
    if case["mend"] == "on":
        yh = _host(y.reshape(xin.shape), case).reshape(x.shape[0], ch)
        keep, TM.WORST = dict(TM.WORST), {}                             # the comparator's own tallies: this file's are kept apart
        try:
            assert len(e["mend"]) == len(statuses)
            for (m, rows, ref), (m2, status) in zip(e["mend"], statuses):
                assert m == m2
                checked = TM._compare(f"{CC.case_id(case)} channel {m}", np.ascontiguousarray(x2[:, m or 0]), rows, ref,
                                      np.ascontiguousarray(yh[:, m or 0]), np.asarray(status), quiet=True)
                SUMMARY["mended_samples"] += checked
            SUMMARY["fp32"] = max(SUMMARY["fp32"], TM.WORST.get("fp32", 0.0))
            SUMMARY["pcm_odd"] += TM.WORST.get("int16", 0) + TM.WORST.get("s24", 0)
        finally:
            TM.WORST = keep
        filled = np.zeros((x.shape[0], ch), bool)
        for c, rows in enumerate(per(got["mended"])):
            for s, l, st in rows:
                if st in FILLED:
                    filled[s:s + l, c] = True
        away = filled & ~allowed                                        # a mended sample no cross-fade reaches is mend_runs' own
        assert away.any() and np.array_equal(_raw(ph)[away], _raw(yh)[away])
        allowed |= filled
    # ---- 2: by parts
    _same(got, parts)
    # ---- 3: the write set
    assert np.array_equal(_raw(ph)[~allowed], _raw(x2)[~allowed]), int((_raw(ph)[~allowed] != _raw(x2)[~allowed]).any(axis=-1).sum())
    assert (_raw(ph)[allowed] != _raw(x2)[allowed]).any()
    if case["layout"] == "each3":
        assert not allowed[:, 1].any() and np.array_equal(_raw(ph)[:, 1], _raw(x2)[:, 1])
    if case["batch"] == 2:
        assert len(got["contexts"]) > 2                                 # several passes
    SUMMARY["cases"] += 1
    return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conceal_file_equals_its_parts_and_its_references(case):
    _check_case(_engine(), case)


ONE = dict(kind="invalid", stype="fp32", layout="one", sr=48000, feed="contexts", clips16="file", mend="on", rel=0, batch=2, input="device")


def test_an_n_by_1_file_equals_its_flattening():
    eng = _engine()
    flat_case = dict(ONE, layout="mono")
    a, b = CC.expected(ONE), CC.expected(flat_case)
    assert np.array_equal(a["x"].reshape(-1).view(np.uint32), b["x"].view(np.uint32))     # one file, two shapes
    one = eng.conceal_file(CC.as_input(a["x"], ONE, eng.device), 48000, **a["kw"])
    mono = eng.conceal_file(CC.as_input(b["x"], flat_case, eng.device), 48000, **b["kw"])
    assert one["patched"].shape == (a["x"].shape[0], 1) and mono["patched"].shape == (a["x"].shape[0],)
    _same(dict(one, patched=one["patched"].reshape(-1)), mono)
    s24_case = dict(ONE, kind="quiet", stype="s24", mend="off")
    c = CC.expected(s24_case)
    one = eng.conceal_file(CC.as_input(c["x"], s24_case, eng.device), 48000, **c["kw"])
    mono = eng.conceal_file(CC.as_input(c["x"].reshape(-1), dict(s24_case, layout="mono"), eng.device), 48000, **c["kw"])
    assert one["patched"].shape == (c["x"].shape[0], 1, 3) and one["patched"].dtype == torch.uint8
    _same(dict(one, patched=one["patched"].reshape(-1, 3)), mono)


@pytest.mark.parametrize("layout", ["mono", "each2"])
def test_a_host_array_equals_a_device_tensor(layout):
    eng = _engine()
    case = dict(kind="any", stype="int16", layout=layout, sr=16000, feed="recording", clips16="resampled", mend="on", rel=1, batch=32, input="host")
    e = CC.expected(case)
    host = eng.conceal_file(CC.as_input(e["x"], case, eng.device), 16000, **e["kw"])
    array = eng.conceal_file(e["x"], 16000, **e["kw"])                   # the numpy array itself
    dev = eng.conceal_file(CC.as_input(e["x"], dict(case, input="device"), eng.device), 16000, **e["kw"])
    assert not CC.as_input(e["x"], case, eng.device).is_cuda and host["patched"].is_cuda
    _same(host, dev)
    _same(array, dev)


@pytest.mark.parametrize("name", sorted(CC.FORBIDDEN))
def test_a_forbidden_pair_is_refused_before_any_launch(name):
    """clips16_feed and invalid_feed are the two this sweep found: patch_file's rules, which conceal_file used to reach only after the
    detection -- and with mend_ms the mending -- had run."""
    eng = _engine()
    stype, sr, kw = CC.FORBIDDEN[name]
    x = CC.forbidden_file(stype, sr).to(eng.device)
    for more in ({}, {"mend_ms": 1.0, "min_ms": 0} if "mend_ms" not in kw else {}):
        eng.ctx.profile_start(100)
        try:
            with pytest.raises(ValueError, match=CC.CONSTRAINTS[name][1]):
                eng.conceal_file(x, sr, **{**kw, **more})
        finally:
            prof = {q["name"]: q["launches"] for q in eng.ctx.profile_stop() if q["launches"] > 0}
        assert prof == {}, (name, more, prof)


def test_zz_the_sweep_in_numbers():
    """Printed for DESIGN.md 4.35.  The references predict no PCM sample at a half-integer; fp32 stays within its bound."""
    wall = time.time() - SUMMARY["t0"]
    print(f"   SUMMARY conceal pairs: {SUMMARY['cases']} cases, {SUMMARY['mended_samples']} mended samples, worst fp32 |gpu - ref| / bound "
          f"{SUMMARY['fp32']:.4f}, PCM half-integer exceptions {SUMMARY['pcm_odd']}, device calls {SUMMARY['gpu_s']:.1f} s, file wall time {wall:.1f} s")
    assert SUMMARY["fp32"] <= 1.0
