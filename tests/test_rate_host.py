"""CPU: the host side of the file-rate repair -- the `long: {rate: ...}` key of predict.yaml, the RateTable builder and
its refusals, the declaration of si_patch_rate / si_rate_table against the Python mirror, and the planning property the route rests on:
generator windows planned from the reach-widened regions keep every tap of every written sample in their kept region."""
import ctypes
import os
import re

import numpy as np
import pytest

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd import native
from speech_inpainting_amd.config import load_predict_config
from tests import rate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _yaml(tmp_path, extra, drop=()):
    import yaml
    data = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "golden", "iea_predict.yaml")))
    for key in drop:
        data.pop(key, None)
    p = tmp_path / "predict.yaml"
    p.write_text(yaml.safe_dump(data) + "\n" + extra)
    return str(p)


def test_predict_yaml_long_rate_key(tmp_path):
    assert load_predict_config(_yaml(tmp_path, "")).long_rate == 22050
    cfg = load_predict_config(_yaml(tmp_path, "long: {}\n"))
    assert cfg.long_rate == 22050 and cfg.long == {"clip_s": 4.0, "context_s": 1.0, "batch": 32}          # the default is today's route
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file}\n"))
    assert cfg.long_rate == "file" and cfg.long == {"clip_s": 4.0, "context_s": 1.0, "batch": 32}
    cfg = load_predict_config(_yaml(tmp_path, "long:\n  rate: 22050\n  clip_s: 1.5\n  context_s: 0.3\n"))
    assert cfg.long_rate == 22050 and cfg.long["clip_s"] == 1.5
    cfg = load_predict_config(_yaml(tmp_path, "long: {rate: file, batch: 2}\ndetect: {threshold: 0.001}\npatch: {fade_ms: 2}\n", drop=("mask",)))
    assert cfg.long_rate == "file" and cfg.detect["threshold"] == 0.001 and cfg.patch_fade_ms == 2.0 and cfg.long["batch"] == 2
    for bad in ("48000", "true", "'22050'", "[file]"):
        with pytest.raises(ValueError, match="long.rate"):
            load_predict_config(_yaml(tmp_path, f"long: {{rate: {bad}}}\n"))
    with pytest.raises(ValueError, match="unknown key `rates` in `long:`"):
        load_predict_config(_yaml(tmp_path, "long: {rates: file}\n"))


def test_rate_table_layout_and_refusals():
    spans = [(100, 50, 0, 4000), (300, 20, 1, 4000)]
    wins = [(0, 0, 512, 2000), (1, 256, 768, 2000)]
    chunks = [(0, 0, 2)]
    t = native.RateTable(spans, wins, chunks, 2, 7, "cpu")
    assert (t.K, t.W, t.Q, t.C, t.fade) == (2, 2, 1, 2, 7)
    h = t.host
    assert h.dtype == np.int32 and h.size == 4 * 2 + 4 * 2 + 3 * 1 + 7 + 1
    assert list(h[:8]) == [100, 300, 50, 20, 0, 1, 4000, 4000] and list(h[8:16]) == [0, 1, 0, 256, 512, 768, 2000, 2000] and list(h[16:19]) == [0, 0, 2]
    assert np.array_equal(h[19:26].view(np.float32), G.fade_ramp(7))
    st = t.struct()
    assert st.struct_size == ctypes.sizeof(native.RateTableStruct) == 6 * 4 + 23 * 8
    base = h.ctypes.data
    assert (st.host_start, st.host_span_lim, st.host_win_ctx, st.host_win_lim, st.host_chunk, st.host_k1) == tuple(base + 4 * o for o in (0, 6, 8, 14, 16, 18))
    assert st.ramp - st.start == 4 * 19 and st.win_lim - st.start == 4 * 14 and (st.num_contexts, st.num_windows, st.num_spans, st.num_chunks, st.fade) == (2, 2, 2, 1, 7)
    empty = native.RateTable([], [], [], 0, 0, "cpu")
    assert empty.host.size == 1 and empty.struct().num_chunks == 0
    with pytest.raises(ValueError, match="span 1"):
        native.RateTable([spans[0], (300, 20, 1)], wins, chunks, 2, 7, "cpu")                       # a region-table row: no lim
    with pytest.raises(ValueError, match="window 0"):
        native.RateTable(spans, [(0, 0, 512), wins[1]], chunks, 2, 7, "cpu")                        # a window without its context's end
    with pytest.raises(ValueError, match="span 0"):
        native.RateTable([(2 ** 31, 50, 0, 4000)], wins, chunks, 2, 7, "cpu")
    with pytest.raises(ValueError, match="chunk 0"):
        native.RateTable(spans, wins, [(0, 0)], 2, 7, "cpu")
    with pytest.raises(ValueError, match="negative"):
        native.RateTable(spans, wins, chunks, 2, -1, "cpu")


def test_header_declares_the_entry_and_the_table_the_mirror_mirrors():
    hdr = open(os.path.join(ROOT, "include", "si_hip.h")).read()
    assert re.search(r"#define SI_ABI_VERSION 3\b", hdr)
    body = re.search(r"typedef struct si_rate_table \{(.*?)\} si_rate_table;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|const int32_t\*|const float\*)\s+([a-z_0-9]+);", body)
    assert [n for _, n in fields] == [n for n, _ in native.RateTableStruct._fields_]
    assert [ctypes.c_int32 if t == "int32_t" else ctypes.c_void_p for t, _ in fields] == [t for _, t in native.RateTableStruct._fields_]
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = re.search(r"int si_patch_rate\((.*?)\);", code, flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "orig", "is_pcm16", "n_file", "sr", "table", "gen", "Lrow", "gain", "filt", "out", "stream"]
    assert "si_patch_rate" in native.EXPORTS
    if os.path.exists(native.LIB_PATH):
        lib = native.load_library()
        assert len(lib.si_patch_rate.argtypes) == len(args) and lib.si_version() == 3
    # the header says what the entry replaces, as its neighbours do
    assert re.search(r"si_patch_rate\s+<-", hdr) and "DESIGN.md 4.16" in hdr


@pytest.mark.parametrize("sr", [8000, 11025, 16000, 44100, 48000])
@pytest.mark.parametrize("rf", [3, 23])
def test_widened_windows_keep_every_tap_in_the_kept_region(sr, rf):
    """One context clip of 200 frames that starts at recording frame 120, gaps near its front, middle and end; hop 256, receptive
    radius rf frames.  The windows planned from gaps.reach_regions22 hold, in their KEPT frames, every 22.05 kHz sample that any
    written file sample's interpolation reads inside [0, lim22); the windows planned from the bare mapped region of a gap that starts on a generator frame do not."""
    hop, start, frames = 256, 120, 200
    P, Q = G.rate_ratio(sr)
    H = R.reach(sr)
    off, L22 = 441 * start, 441 * frames
    t_out = (L22 - 400) // hop
    lim22 = off + t_out * hop
    own = [(2, 3), (90, 5), (96, 2), (190, 6)]
    fade_f = G.file_fade(5.0, sr)
    spans = G.file_spans([(start + p, l) for p, l in own], sr)
    lim_f = G.file_lim(lim22, sr)
    regs = G.file_regions(spans, [lim_f] * len(spans), fade_f)
    assert all(r is not None for r in regs) and regs[-1][1] <= lim_f

    def missing(regions22, regs=regs):
        local = [(a - off, b - off) for a, b in regions22]
        wins, which = G.plan_patch_windows(local, t_out, hop, rf)
        bad = 0
        for (a, b), w in zip(regs, which):
            k0, k1 = G.kept_region(*wins[w], t_out, rf)
            lo, hi = off + k0 * hop, off + k1 * hop
            for i in (a, b - 1):                                        # n is monotonic in i: the two ends bound every sample's taps
                n = i * P // Q
                taps = [j for j in (n - (H - 1), n + H) if 0 <= j < lim22]
                bad += sum(not lo <= j < hi for j in taps)
        return bad

    assert missing(G.reach_regions22(regs, sr, H, -2 ** 62, lim22)) == 0
    # a region whose first sample sits on a frame boundary of the generator: without the reach the kept frames begin AT that sample
    i0 = -(-(off + 40 * hop) * Q // P)
    edge = [(i0, i0 + 50)]
    assert 0 <= i0 * P // Q - (off + 40 * hop) < H - 1
    assert missing([(a * P // Q, (b - 1) * P // Q + 1) for a, b in edge], edge) > 0
    assert missing(G.reach_regions22(edge, sr, H, -2 ** 62, lim22), edge) == 0
