"""Dropout detection on the device: si_quiet_runs against the numpy reference of tests/detect_ref.py -- the total and
every (start, len) row, exact integer equality -- engine.find_quiet_runs / find_gaps / conceal_recording, and the `detect:` key of
predict.yaml.  The route adds no arithmetic, so conceal_recording is compared bit for bit with patch_recording on the known gaps.

The route's common shape is tests/test_gpu_long.py's: a recording of 300 frames + 123 samples (132 423 samples), clips of 75 frames,
15 frames of context, GAPS below.  Two of GAPS lie ONE frame apart, and find_gaps' default merge_frames (2 * the cross-fade's frames
= 2) joins them into (100, 10) by design; the tests that must get GAPS back pass merge_frames=1 and assert the default's answer too."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import detect_ref as D
from tests.cases import _patch_engine as _engine

pytestmark = pytest.mark.gpu

N_REC, TAIL, CLIP, CTX = 300, 123, 75, 15
N22 = N_REC * 441 + TAIL
N16 = -(-N22 * 320 // 441)
GAPS = [(2, 3), (100, 5), (106, 4), (140, 6), (292, 5)]
KW = dict(clip_frames=CLIP, min_context=CTX)
TORCH = {np.float32: torch.float32, np.int16: torch.int16}
SENTINEL = -7


def _i32(t):
    return t.contiguous().view(torch.int32)


def _runs(ctx, x, thr, min_len, max_runs=4096, offset=0):
    """si_quiet_runs on the host array x, placed `offset` elements into a device buffer -> (total, rows written, the rows past them)."""
    buf = torch.zeros(offset + x.size, dtype=TORCH[x.dtype.type], device=ctx.device)
    buf[offset:] = torch.from_numpy(x)
    view = buf[offset:]
    assert view.data_ptr() == buf.data_ptr() + offset * x.itemsize
    runs = torch.full((max_runs + 8, 2), SENTINEL, dtype=torch.int32, device=ctx.device)
    _, n_runs = ctx.quiet_runs(view, thr, min_len, max_runs, runs=runs)
    total = int(n_runs.item())
    rows = runs.cpu().numpy()
    k = min(total, max_runs)
    return total, rows[:k], rows[k:]


def _check(ctx, x, thr, min_len, what, **kw):
    want = D.quiet_runs_ref(x, thr, min_len)
    total, rows, rest = _runs(ctx, x, thr, min_len, **kw)
    assert total == len(want), (what, total, len(want))
    assert len(rows) == min(total, kw.get("max_runs", 4096)) and np.array_equal(rows, want[:len(rows)]), (what, rows[:8].tolist(), want[:8].tolist())
    assert np.all(rest == SENTINEL), what
    return want


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("n", D.SEAM_N)
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_runs_at_the_chunk_seams(dtype, n):
    """Every placement of tests/detect_ref.py::seam_cases: runs crossing, ending on and starting on a chunk seam, whole quiet chunks
    inside a run, runs from sample 0 and reaching n, all quiet, all loud, lengths min_len - 1 / min_len / min_len + 1, 1024 runs in a
    chunk; the values hold |x| == thr, NaN, +-inf, -0.0, subnormals and -32768."""
    ctx = _engine().ctx
    found = 0
    for name, q, min_len in D.seam_cases(n):
        found += len(_check(ctx, D.materialize(q, dtype, n), D.THR[dtype], min_len, (n, name)))
    assert found > 0
    if n >= 2048:
        assert len(_check(ctx, D.materialize(np.arange(n) % 2 == 0, dtype), D.THR[dtype], 1, "alternating")) >= 1024


@pytest.mark.parametrize("dtype,offsets", [(np.float32, (1, 2, 3)), (np.int16, (1, 3, 7, 8))])
def test_a_base_pointer_off_the_16_byte_grid(dtype, offsets):
    """Views that start 1, 2, 3 floats / 1, 3, 7 int16 into an allocation take the staged path; 8 int16 = 16 bytes is aligned again."""
    ctx = _engine().ctx
    for n in (7, 2049, 4101, 6144):
        for name, q, min_len in D.seam_cases(n):
            x = D.materialize(q, dtype, n + 1)
            for off in offsets:
                _check(ctx, x, D.THR[dtype], min_len, (n, name, off), offset=off)


def test_value_edges_at_threshold_zero_and_above():
    ctx = _engine().ctx
    y = np.array([np.nan, -0.0, 1e-40, np.inf, -np.inf, 0.0, -1e-40, 0.0, 0.0, 1.0], dtype=np.float32)
    assert _check(ctx, y, 0.0, 1, "thr 0").tolist() == [[1, 1], [5, 1], [7, 2]]                  # a subnormal is loud at thr = 0
    assert _check(ctx, y, 1e-38, 1, "thr 1e-38").tolist() == [[1, 2], [5, 4]]
    assert _check(ctx, y, float("inf"), 1, "thr inf").tolist() == [[1, 9]]                       # NaN stays loud
    x = np.array([0, 0, 1, 0, 0.5, 0.25, 0, 0, 0, 2, 0], dtype=np.float32)
    assert _check(ctx, x, 0.25, 1, "== thr").tolist() == [[0, 2], [3, 1], [5, 4], [10, 1]]
    p = np.array([-32768, 3, -3, 4, 0, 32767, -32768], dtype=np.int16)
    assert _check(ctx, p, 3.0, 1, "pcm").tolist() == [[1, 2], [4, 1]]
    assert _check(ctx, p, 32767.0, 1, "pcm 32767").tolist() == [[1, 5]]                          # |-32768| = 32768, taken in int32
    assert _check(ctx, p, 32768.0, 1, "pcm 32768").tolist() == [[0, 7]]
    assert _check(ctx, p, 0.0, 1, "pcm 0").tolist() == [[4, 1]]


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
@pytest.mark.parametrize("density", [0.5, 0.05, 0.002])
def test_seeded_random_patterns(dtype, density):
    """Geometric run lengths at three densities over five chunks and 77 samples, with one planted run that holds three whole quiet
    chunks in a row; the same call twice gives the same bytes."""
    ctx = _engine().ctx
    n = 5 * D.CHUNK + 77
    q = D.random_mask(n, density, int(density * 1000))
    q2 = q | D.mask_of(n, [(D.CHUNK - 48, 4 * D.CHUNK + 100)])
    for mask in (q, q2):
        x = D.materialize(mask, dtype, 11)
        for min_len in (1, 3, 64, 3000):
            want = _check(ctx, x, D.THR[dtype], min_len, (density, min_len))
            assert mask is q or int(want[:, 1].max()) >= 3 * D.CHUNK + 148                      # the planted run, whole chunks 1 .. 3 inside it
    a = _runs(ctx, x, D.THR[dtype], 1, max_runs=8192)
    b = _runs(ctx, x, D.THR[dtype], 1, max_runs=8192)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------ 3
def test_the_carry_scan_across_its_own_tile_seam():
    """1027 chunks and 5 samples: the carry pass takes two tiles of D.CARRY_TILE chunks.  One run spans the tile seam with whole quiet
    chunks on both sides of it, runs end on either side of it, and (second mask) a run ends exactly on it."""
    ctx = _engine().ctx
    n, seam, q, q2 = D.tile_seam_case()
    assert -(-n // D.CHUNK) > D.CARRY_TILE
    for k, mask in enumerate((q, q2)):
        for dtype in (np.float32, np.int16):
            x = D.materialize(mask, dtype, k)
            for min_len in (1, 64):
                want = _check(ctx, x, D.THR[dtype], min_len, ("tile seam", k, min_len), max_runs=1 << 18)
                assert [seam - D.CHUNK - 1000, (2 * D.CHUNK + 1200, D.CHUNK + 1000)[k]] in want.tolist()


# ------------------------------------------------------------------------------------------------------------ 4
def test_max_runs():
    eng = _engine()
    ctx = eng.ctx
    x = D.materialize(np.arange(4101) % 2 == 0, np.float32)
    want = D.quiet_runs_ref(x, D.THR[np.float32], 1)
    assert len(want) == 2051
    for cap in (100, 2050, 2051, 2052, 1):
        total, rows, rest = _runs(ctx, x, D.THR[np.float32], 1, max_runs=cap)
        assert total == 2051 and np.array_equal(rows, want[:cap]) and np.all(rest == SENTINEL), cap
    dev = torch.from_numpy(x).to(eng.device)
    runs, n_runs = ctx.quiet_runs(dev, D.THR[np.float32], 1, 0)                                  # max_runs = 0 counts only
    assert runs is None and int(n_runs.item()) == 2051
    got = eng.find_quiet_runs(dev, D.THR[np.float32], 1, max_runs=2051)
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(eng.find_quiet_runs(x, D.THR[np.float32]).cpu().numpy(), want)         # a host array, the default cap
    with pytest.raises(ValueError, match=r"2051 runs .* more than max_runs = 100"):
        eng.find_quiet_runs(dev, D.THR[np.float32], 1, max_runs=100)
    assert eng.find_quiet_runs(dev, D.THR[np.float32], 2).shape == (0, 2)


# ------------------------------------------------------------------------------------------------------------ 5
def test_refusals_come_before_any_launch():
    ctx = _engine().ctx
    lib, h, dev = ctx.lib, ctx._h, ctx.device
    x = torch.zeros(4096, device=dev)
    runs = torch.full((16, 2), SENTINEL, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    good = dict(x=x, pcm=0, n=4096, thr=0.0, min_len=1, runs=runs, max_runs=16, cnt=cnt)
    cases = [(dict(x=None), "x is NULL"), (dict(cnt=None), "n_runs is NULL"), (dict(runs=None), "runs is NULL with max_runs = 16"),
             (dict(n=0), "n = 0 samples"), (dict(n=-5), "n = -5 samples"), (dict(n=2 ** 31 - 1 - 2047), "n = 2147481600 samples"),
             (dict(n=2 ** 31 - 1), "n = 2147483647 samples"), (dict(thr=-1e-9), "threshold = -1e-09 is negative or NaN"),
             (dict(thr=float("nan")), "threshold = -?nan is negative or NaN"), (dict(min_len=0), "min_len = 0 samples"),
             (dict(min_len=-3), "min_len = -3 samples"), (dict(max_runs=-1), "max_runs = -1 is negative")]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for change, msg in cases:
        a = {**good, **change}
        ctx.profile_start(100)
        rc = lib.si_quiet_runs(h, P(a["x"]), a["pcm"], a["n"], a["thr"], a["min_len"], P(a["runs"]), a["max_runs"], P(a["cnt"]), stream)
        launched = [e for e in ctx.profile_stop() if e["launches"] > 0]
        err = lib.si_last_error(h).decode()
        assert rc == -1 and launched == [], (change, rc, launched)                               # SI_EINVAL
        assert __import__("re").search("si_quiet_runs: " + msg, err), (change, err)
    torch.cuda.synchronize()
    assert bool((runs == SENTINEL).all()) and int(cnt.item()) == SENTINEL
    # the same arguments unchanged are served, under the detector's own family names
    ctx.profile_start(100)
    rc = lib.si_quiet_runs(h, P(x), 0, 4096, 0.0, 1, P(runs), 16, P(cnt), stream)
    prof = {e["name"]: e["launches"] for e in ctx.profile_stop()}
    assert rc == 0 and prof == {"detect_bits": 1, "detect_carry": 1, "detect_count": 1, "detect_offsets": 1, "detect_emit": 1}, prof
    assert int(cnt.item()) == 1 and runs[0].tolist() == [0, 4096]


# ------------------------------------------------------------------------------------------------------------ 6, 7
def _recording(seed=41):
    from speech_inpainting_amd import synth
    return synth.synth_wave(1, N22, seed, sr=22050)[0].cuda(), synth.synth_wave(1, N16, seed + 1)[0].cuda()


def _zeroed(wave, spf, extra=()):
    out = wave.clone()
    for p, l in GAPS:
        out[spf * p:spf * (p + l)] = 0
    for a, b in extra:
        out[a:b] = 0
    return out


@pytest.mark.parametrize("voc", ["fp32", "fp16"])
def test_conceal_recording_equals_patch_recording_on_the_known_gaps(voc):
    """GAPS zeroed in the recording: find_gaps at threshold 0 returns exactly GAPS, and conceal_recording equals
    patch_recording(that recording, GAPS) bit for bit.  The synthetic recording has no exact-zero sample of its own (asserted)."""
    eng = _engine(voc)
    wave22, _ = _recording()
    assert int((wave22 == 0).sum()) == 0
    rec = _zeroed(wave22, 441)
    found = eng.find_gaps(rec, threshold=0.0, merge_frames=1)
    assert found["gaps"] == GAPS and found["skipped"] == []
    assert found["runs"].tolist() == [[441 * p, 441 * l] for p, l in GAPS]
    assert eng.find_gaps(rec, threshold=0.0)["gaps"] == [(2, 3), (100, 10), (140, 6), (292, 5)]  # the default joins gaps one frame apart
    want = eng.patch_recording(rec, GAPS, fade=110, pcm=True, **KW)
    got = eng.conceal_recording(rec, threshold=0.0, merge_frames=1, fade=110, pcm=True, **KW)
    torch.cuda.synchronize()
    assert got["gaps"] == GAPS and got["skipped"] == [] and got["contexts"] == want["contexts"] and len(want["contexts"]) == 4
    assert torch.equal(_i32(got["patched"]), _i32(want["patched"])), int((got["patched"] != want["patched"]).sum())
    assert torch.equal(got["patched_pcm"], want["patched_pcm"]) and torch.equal(got["labels"], want["labels"]) and got["label_off"] == want["label_off"]
    for p, l in GAPS:
        assert bool((got["patched"][441 * p:441 * (p + l)] != 0).any())


def test_edges_rates_and_nothing_to_find():
    eng = _engine()
    wave22, wave16 = _recording()
    # leading and trailing padding: both runs come back as "edge", and the output there is the input's bits
    rec = _zeroed(wave22, 441, [(0, 300), (N22 - 1000, N22)])
    rec.view(torch.int32)[7] = -2 ** 31                                                          # -0.0 is quiet, and survives
    got = eng.conceal_recording(rec, merge_frames=1, **KW)
    assert got["gaps"] == GAPS and got["skipped"] == [(0, 1, "edge"), (298, 2, "edge")]
    want = eng.patch_recording(rec, GAPS, **KW)
    assert torch.equal(_i32(got["patched"]), _i32(want["patched"]))
    assert torch.equal(_i32(got["patched"][:300]), _i32(rec[:300])) and torch.equal(_i32(got["patched"][-1000:]), _i32(rec[-1000:]))
    # the file's own samples at another rate: the 16 kHz recording zeroed at [320 p, 320 (p + l)), as fp32 and as int16
    rec16 = _zeroed(wave16, 320)
    assert int((wave16 == 0).sum()) == 0
    found = eng.find_gaps(rec16, sr=16000, merge_frames=1, n_rec_frames=N_REC)
    assert found["gaps"] == GAPS and found["runs"].tolist() == [[320 * p, 320 * l] for p, l in GAPS]
    pcm16 = (rec16 * 32767).to(torch.int16)
    ref16 = D.quiet_runs_ref(pcm16.cpu().numpy(), 0.0, 80)
    assert eng.find_gaps(pcm16, sr=16000, merge_frames=1, n_rec_frames=N_REC)["runs"].tolist() == ref16.tolist()
    plain = _zeroed(wave22, 441)
    via16 = eng.conceal_recording(plain, detect_on=rec16, sr=16000, merge_frames=1, **KW)
    assert via16["gaps"] == GAPS and torch.equal(_i32(via16["patched"]), _i32(eng.patch_recording(plain, GAPS, **KW)["patched"]))
    # nothing to find: an exact copy, and only the detector's kernels in the profile
    wave22.view(torch.int32)[5] = 0x7fc12345
    eng.ctx.profile_start(100)
    none = eng.conceal_recording(wave22, **KW)
    prof = {e["name"]: e["launches"] for e in eng.ctx.profile_stop() if e["launches"] > 0}
    torch.cuda.synchronize()
    assert set(prof) == {"detect_bits", "detect_carry", "detect_count", "detect_offsets", "detect_emit"}, prof
    assert none["gaps"] == [] and none["skipped"] == [] and none["contexts"] == [] and none["label_off"] == [0]
    assert none["patched"].data_ptr() != wave22.data_ptr() and torch.equal(_i32(none["patched"]), _i32(wave22))


# ------------------------------------------------------------------------------------------------------------ 8
def test_predict_entry_point_with_a_detect_key(tmp_path, monkeypatch, capsys):
    """predict.py on a 6 s int16 file with three zeroed stretches, `long:` and `detect:`.  The expected frames come from the numpy
    reference and runs_to_gaps on the file itself: the synthetic int16 file has isolated zero samples of its own, and one next to a
    zeroed stretch legitimately widens a cover."""
    import joblib
    from scipy.io import wavfile
    from sklearn.cluster import MiniBatchKMeans
    from speech_inpainting_amd import gaps as G
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.arch import HubertArch, VocoderArch
    from speech_inpainting_amd.predict import main

    harch, varch = HubertArch.base(), VocoderArch.v1()
    hsd, gsd, cb = synth.synth_hubert_state(harch, pos_conv_style="legacy"), synth.synth_generator_state(varch), synth.synth_codebook(100)
    (tmp_path / "trained_models").mkdir()
    torch.save(dict(hsd), tmp_path / "trained_models" / "save_checkpoint.pt")
    (tmp_path / "hifi_gan" / "LJ_V1").mkdir(parents=True)
    torch.save({"generator": dict(gsd)}, tmp_path / "hifi_gan" / "LJ_V1" / "generator_v1")
    (tmp_path / "hifi_gan" / "LJ_V1" / "config.json").write_text(json.dumps(dict(
        resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
        resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, num_mels=80, sampling_rate=22050, seed=1234)))
    kdir = tmp_path / "kmeans" / "km_model_100"
    kdir.mkdir(parents=True)
    km = MiniBatchKMeans(n_clusters=100)
    km.cluster_centers_ = cb.numpy()
    joblib.dump(km, kdir / "model.km")
    n22 = 6 * 22050 + 123
    pcm_in = (synth.synth_wave(1, n22, 5, sr=22050)[0].numpy() * 32767).astype(np.int16)
    stretches = ((441 * 25, 441 * 31), (441 * 100 + 37, 441 * 104 + 200), (441 * 250 - 5, 441 * 262))
    for a, b in stretches:
        pcm_in[a:b] = 0
    (tmp_path / "wavs").mkdir()
    wavfile.write(tmp_path / "wavs" / "call.wav", 22050, pcm_in)
    (tmp_path / "predict.yaml").write_text(f"""
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: '{tmp_path}/wavs/call.wav', save_pred: '{tmp_path}/prediction'}}}}
long: {{clip_s: 1.5, context_s: 0.3, batch: 2}}
detect: {{min_ms: 5}}
device: {{index: 0}}
hifi_gan: {{checkpoint_file: '{tmp_path}/hifi_gan/LJ_V1/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: '{tmp_path}/trained_models/save_checkpoint.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: '{tmp_path}/kmeans/', km_model_path: '{tmp_path}/kmeans/'}}}}
""")
    gaps, skipped = G.runs_to_gaps(D.quiet_runs_ref(pcm_in, 0.0, 110).tolist(), n22, 22050, 300, merge_frames=2)
    assert len(gaps) == 3 and skipped == []
    assert all(p <= a // 441 and -(-b // 441) <= p + l <= -(-b // 441) + 1 for (p, l), (a, b) in zip(gaps, stretches))
    monkeypatch.chdir(tmp_path)
    assert main([]) == 0
    out = tmp_path / "prediction" / "call"
    assert sorted(p.name for p in out.iterdir()) == ["gaps.json", "masked.wav", "orig.wav", "patched.wav"]
    assert json.loads((out / "gaps.json").read_text()) == {"gaps": [list(g) for g in gaps], "skipped": []}
    printed = capsys.readouterr().out
    for k, (p, l) in enumerate(gaps):
        assert f"Detected gap {k} = frames [{p}, {p + l}) = {p * 0.02:.2f} s .. {(p + l) * 0.02:.2f} s" in printed
        assert f"Predicted codewords, gap {k} = frames [{p}, {p + l})" in printed
    files = {}
    for f in ("orig.wav", "masked.wav", "patched.wav"):
        sr, files[f] = wavfile.read(out / f)
        assert sr == 22050 and files[f].dtype == np.int16 and len(files[f]) == n22, f
    assert np.array_equal(files["orig.wav"], pcm_in)
    keep = np.ones(n22, dtype=bool)
    zeroed = pcm_in.copy()
    for p, l in gaps:
        keep[441 * p - 110:441 * (p + l) + 110] = False                   # the default fade: 5 ms
        zeroed[441 * p:441 * (p + l)] = 0
        assert not np.array_equal(files["patched.wav"][441 * p:441 * (p + l)], pcm_in[441 * p:441 * (p + l)])
    assert np.array_equal(files["patched.wav"][keep], pcm_in[keep])
    assert np.array_equal(files["masked.wav"], zeroed)
