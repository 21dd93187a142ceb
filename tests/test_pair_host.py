"""CPU: the host side of DESIGN.md 4.26 -- the LDS a si_cut_pair launch asks for at every permitted rate, the two declarations against
their ctypes mirrors, the `long: {clips16: ...}` key of predict.yaml with its refusals, and the routing of clips16 through patch_file,
conceal_file and predict.py."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from speech_inpainting_amd import predict as P
from speech_inpainting_amd.config import load_predict_config
from speech_inpainting_amd.engine import InpaintingEngine
from tests import pair_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("si_cut_pair", "si_cut_pair_ch")


# ------------------------------------------------------------------------------------------------------------ LDS
def _reach(sr, target):
    """Taps per wing of kaiser_best's table (32 769 entries at 512 per zero crossing) towards `target`: ceil(nwin / int(scale 512))."""
    return 0 if sr == target else -(-32769 // int(min(1.0, float(target) / sr) * 512))


def test_a_tile_s_staged_samples_fit_the_lds_at_every_permitted_rate():
    """ceil(F sr / 50) + 2 + 2 max(H22, H16) floats per workgroup: at 192 kHz with one frame per tile 3840 + 2 + 2 * 781 = 5404; the
    largest launch stays under the 64 KB a launch gets without asking for more."""
    assert (_reach(192000, 16000), _reach(192000, 22050), _reach(48000, 16000), _reach(16000, 16000)) == (781, 565, 193, 0)
    for sr in (48000, 192000, 8000):
        assert (_reach(sr, 16000), _reach(sr, 22050)) == (PR.reach(sr, 16000), PR.reach(sr, 22050))
    worst = 0
    for sr in list(range(4000, 192001, 25)) + [4001, 11025, 44100, 191999]:
        if sr == 22050:
            continue
        floats = native.cut_pair_lds_floats(sr, _reach(sr, 22050), _reach(sr, 16000))
        assert floats == -(-native.CUT_PAIR_FRAMES * sr // 50) + 2 + 2 * max(_reach(sr, 22050), _reach(sr, 16000))
        worst = max(worst, floats)
    assert 4 * worst <= 65536 < 160 * 1024
    if native.CUT_PAIR_FRAMES == 1:
        assert worst == 5404 == native.cut_pair_lds_floats(192000, 565, 781) == PR.lds_floats(192000, 1)


def test_the_two_rows_of_a_frame_start_at_one_file_position():
    """441 f Q22 / P22 = 320 f Q16 / P16 = f sr / 50: what lets one staged range serve both rates."""
    for sr in (4000, 8000, 11025, 16000, 32000, 44100, 48000, 96000, 192000, 4001, 191999):
        P22, Q22 = G.rate_ratio(sr)
        P16, Q16 = G.rate_ratio16(sr)
        assert (P16, Q16) == (16000 // np.gcd(16000, sr), sr // np.gcd(16000, sr))
        for f in (0, 1, 7, 29999, 4_000_000):
            assert 441 * f * Q22 // P22 == 320 * f * Q16 // P16 == f * sr // 50
    assert G.rate_ratio16(16000) == (1, 1) and G.rate_ratio16(48000) == (1, 3) and G.rate_ratio16(44100) == (160, 441)
    with pytest.raises(ValueError, match="outside"):
        G.rate_ratio16(3999)


# ------------------------------------------------------------------------------------------------------------ the ABI
def _declaration(hdr, name):
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return [a.strip() for a in re.search(rf"int {name}\((.*?)\);", code, flags=re.S).group(1).split(",")]


def test_header_declares_the_entries_the_mirror_calls():
    hdr = open(os.path.join(ROOT, "include", "si_hip.h")).read()
    assert re.search(r"#define SI_ABI_VERSION 3\b", hdr)
    assert int(re.search(r"#define SI_CUT_PAIR_FRAMES (\d+)\b", hdr).group(1)) == native.CUT_PAIR_FRAMES
    mono, inter = _declaration(hdr, "si_cut_pair"), _declaration(hdr, "si_cut_pair_ch")
    names = lambda args: [a.split()[-1].lstrip("*") for a in args]
    assert names(mono) == ["ctx", "x", "is_pcm16", "n_file", "sr", "host_frame", "frame", "C", "L22", "L16", "filt22", "filt16", "out22", "out16",
                           "stream"]
    assert names(inter) == names(mono)[:4] + ["channels", "channel"] + names(mono)[4:]
    assert inter[4:6] == ["int channels", "int channel"]
    for name, args in zip(NEW, (mono, inter)):
        assert name in native.EXPORTS
        if os.path.exists(native.LIB_PATH):
            lib = native.load_library()
            argtypes = getattr(lib, name).argtypes
            assert len(argtypes) == len(args) and lib.si_version() == 3
            assert [t is ctypes.c_int32 for t in argtypes] == [not (("*" in a) or a.startswith("si_stream_t")) for a in args]
    # the header says what the entries stand for, as their neighbours do, and cites the reference's two loads
    assert re.search(r"si_cut_pair / si_cut_pair_ch\s+<-", hdr) and "DESIGN.md 4.26" in hdr
    block = hdr[hdr.index("DESIGN.md 4.26"):hdr.index("int si_cut_pair(")]
    assert "I_ea/predict.py:79-80" in block and "SI_EINVAL before any launch" in block
    src = open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "rate_feed_kernels.hip")).read()
    assert "cut_pair_kernel<T, decltype(inter)::value, decltype(clean)::value>" in src and "si_with_flag(ch > 0, [&](auto inter)" in src and "RF_PAIR_FRAMES" in src


# ------------------------------------------------------------------------------------------------------------ predict.yaml
def _yaml(tmp_path, extra):
    import yaml
    data = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "golden", "iea_predict.yaml")))
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_long_clips16_key(tmp_path):
    for text in ("", "long: {}\n", "long: {rate: file}\n", "long: {rate: file, feed: contexts}\n"):
        assert load_predict_config(_yaml(tmp_path, text)).long_clips16 == "resampled"              # the default is today's route
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file, feed: contexts, clips16: file}\n"))
    assert cfg.long_clips16 == "file" and cfg.long_feed == "contexts" and cfg.long_rate == "file"
    assert cfg.long == {"clip_s": 4.0, "context_s": 1.0, "batch": 32}                               # cfg.long keeps its shape
    cfg = load_predict_config(_yaml(tmp_path, "long: {clips16: file, batch: 2, feed: contexts, rate: file}\n"))   # in any order
    assert cfg.long_clips16 == "file" and cfg.long["batch"] == 2
    assert load_predict_config(_yaml(tmp_path, "long: {rate: file, feed: contexts, clips16: resampled}\n")).long_clips16 == "resampled"
    assert load_predict_config(_yaml(tmp_path, "long: {clips16: resampled}\n")).long_clips16 == "resampled"
    for bad in ("direct", "true", "16000", "[file]"):
        with pytest.raises(ValueError, match="long.clips16 = "):
            load_predict_config(_yaml(tmp_path, f"long: {{rate: file, feed: contexts, clips16: {bad}}}\n"))
    for text in ("long: {clips16: file}\n", "long: {rate: file, clips16: file}\n", "long: {rate: file, feed: recording, clips16: file}\n"):
        with pytest.raises(ValueError, match="long.clips16 = file needs `feed: contexts`"):
            load_predict_config(_yaml(tmp_path, text))
    with pytest.raises(ValueError, match=r"unknown key `clips` in `long:` \(it takes clip_s, context_s, batch, rate, feed\) and, with feed: contexts, clips16"):
        load_predict_config(_yaml(tmp_path, "long: {clips: file}\n"))


# ------------------------------------------------------------------------------------------------------------ routing
def test_conceal_file_passes_clips16_on_off_its_default_alone():
    calls = []

    def patch_file(*a, **kw):
        calls.append(kw)
        return {"patched": torch.zeros(4)}

    eng = types.SimpleNamespace(device=torch.device("cpu"), recording_frames=lambda *a: (100, 100), patch_file=patch_file,
                                find_gaps=lambda *a, **kw: {"gaps": [], "skipped": [], "runs": None})
    x = torch.zeros(48000)
    InpaintingEngine.conceal_file(eng, x, 48000, feed="contexts", clips16="file")
    assert calls[-1]["clips16"] == "file" and calls[-1]["feed"] == "contexts"
    InpaintingEngine.conceal_file(eng, x.reshape(-1, 2), 48000, feed="contexts", clips16="file", detect="each")
    assert calls[-1]["clips16"] == "file" and calls[-1]["channel_gaps"] == [[], []]
    InpaintingEngine.conceal_file(eng, x, 48000, feed="contexts")
    assert "clips16" not in calls[-1]                                                               # the call of before
    InpaintingEngine.conceal_file(eng, x, 48000, feed="contexts", clips16="resampled")
    assert "clips16" not in calls[-1]


def test_patch_file_refuses_clips16_before_any_work():
    eng = types.SimpleNamespace(device=torch.device("cpu"), _need=lambda **kw: None)
    x = torch.zeros(48000)
    with pytest.raises(ValueError, match="clips16 = 'direct': 'resampled' or 'file'"):
        InpaintingEngine.patch_file(eng, x, 48000, [(10, 3)], feed="contexts", clips16="direct")
    with pytest.raises(ValueError, match="clips16 = 'file' needs feed = 'contexts'"):
        InpaintingEngine.patch_file(eng, x, 48000, [(10, 3)], clips16="file")
    with pytest.raises(ValueError, match="clips16 = 'file' needs feed = 'contexts'"):
        InpaintingEngine.patch_file(eng, x, 48000, [(10, 3)], feed="recording", clips16="file")
    eng._patch_file_channels = lambda *a, **kw: InpaintingEngine._patch_file_channels(eng, *a, **kw)
    with pytest.raises(ValueError, match="clips16 = 'file' needs feed = 'contexts'"):
        InpaintingEngine.patch_file(eng, x.reshape(-1, 2), 48000, [(10, 3)], feed="recording", clips16="file")


def test_predict_passes_the_key_on_and_records_it(tmp_path):
    assert P.clips16_keywords(types.SimpleNamespace(long_clips16="file")) == {"clips16": "file"}
    assert P.clips16_keywords(types.SimpleNamespace(long_clips16="resampled")) == {}
    assert P.clips16_keywords(types.SimpleNamespace()) == {}
    from scipy.io import wavfile
    engine = types.SimpleNamespace(recording_frames=lambda n22, clip: (100, 100),
                                   find_gaps=lambda *a, **kw: {"gaps": [(10, 3)], "skipped": [], "runs": None})
    wavfile.write(tmp_path / "f.wav", 48000, np.zeros(48000, dtype=np.int16))
    for clips16, extra in (("file", {"clips16": "file"}), ("resampled", {})):
        cfg = types.SimpleNamespace(wave_path=str(tmp_path / "f.wav"), detect={"threshold": 0.0, "min_ms": 5.0, "max_ms": 400.0, "pad_frames": 0},
                                    detect_dead=None, detect_level=None, long_clips16=clips16)
        assert P._detect_gaps(cfg, engine, np.zeros(48000, np.float32), 48000, 22050, 110, 200, 50, str(tmp_path)) == [(10, 3)]
        assert json.loads((tmp_path / "gaps.json").read_text()) == {"gaps": [[10, 3]], "skipped": [], **extra}
