"""Packed 24-bit PCM off the device: pack / unpack, the seeded unpack mistakes, the scaling law on the CPU references,
WAV I/O, the `pcm24:` key of predict.yaml and the engine's shape refusals."""
import os
import struct
import wave

import numpy as np
import pytest
import torch

from speech_inpainting_amd import audio
from tests import s24_ref as S

_CASES = {}


def _cases(name):
    if name not in _CASES:
        _CASES[name] = getattr(S, name)()
    return _CASES[name]


def test_round_trips():
    rng = np.random.default_rng(0)
    v = np.concatenate([S.SPECIAL, rng.integers(S.LO, S.HI + 1, 5000).astype(np.int32)]).reshape(-1, 2)
    b = S.pack(v)
    assert b.shape == (v.shape[0], 2, 3) and b.dtype == np.uint8
    assert np.array_equal(S.unpack(b), v) and np.array_equal(audio.unpack_s24(b), v) and np.array_equal(audio.pack_s24(v), b)
    assert audio.unpack_s24(b).dtype == np.int32
    assert np.array_equal(S.image(v).astype(np.float64) * 2.0 ** 23, v)                         # the image is exact
    assert np.array_equal(S.store(S.image(v)), v)                                               # ... and the store rule gives it back
    assert S.store(np.float32([1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 0.99999994, 2.0 ** -24, -(2.0 ** -24)])).tolist() == \
        [S.HI, S.LO, S.HI, S.LO, 0, S.HI, S.LO, S.HI - 0, 0, 0]
    for bad in (np.array([S.HI + 1]), np.array([S.LO - 1]), np.array([0.5])):
        with pytest.raises(ValueError, match="pack_s24"):
            audio.pack_s24(bad)
    with pytest.raises(ValueError, match="unpack_s24"):
        audio.unpack_s24(np.zeros((4, 2), np.uint8))


@pytest.mark.parametrize("bug", S.MISTAKES)
def test_each_unpack_mistake_is_caught(bug):
    """A decoder with the mistake seeded changes the expected rows of at least one case of the value tables."""
    caught = []
    for c in _cases("value_cases") + _cases("channel_value_cases"):
        wrong = S.unpack(S.pack(c.v), bug)
        if np.array_equal(wrong, c.v):
            continue
        if not np.array_equal(S.expected(c, wrong)[0], S.expected(c)[0]):
            caught.append(c.name)
    assert caught, bug


@pytest.mark.parametrize("table", ["lifted_quiet_cases", "lifted_dead_cases", "lifted_level_cases"])
def test_the_scaling_law_on_the_cpu(table):
    """Each lifted case's reference on the fp32 image reproduces the int16 case's rows, and T_s24 = 256 T_int16 = T_F 2^23."""
    cases = _cases(table)
    assert len(cases) >= 90
    for c in cases:
        rows, T = S.expected(c)
        assert np.array_equal(rows, c.rows), c.name
        assert T is None or np.float32(T).tobytes() == np.float32(c.T).tobytes(), (c.name, T, c.T)
    assert sum(len(c.rows) for c in cases) > 100


@pytest.mark.parametrize("ch,n", [(1, 5), (1, 6), (2, 7), (3, 5), (3, 4)])
def test_wav_io(tmp_path, ch, n):
    """Odd and even byte counts, mono, 2 and 3 channels: read back by the project's reader, stdlib wave and scipy (v * 256 in int32)."""
    from scipy.io import wavfile
    rng = np.random.default_rng(10 * ch + n)
    v = rng.integers(S.LO, S.HI + 1, size=(n, ch)).astype(np.int32)
    v[0, 0], v[-1, -1] = S.LO, S.HI
    b = audio.pack_s24(v)
    path = str(tmp_path / "a.wav")
    audio.write_wav_s24(path, b if ch > 1 else b[:, 0], 44100)
    raw = 3 * n * ch
    assert os.path.getsize(path) == 44 + raw + (raw & 1)                                         # the pad byte when 3 n ch is odd
    data, sr, got_ch = audio.read_wav_pcm(path)
    assert sr == 44100 and got_ch == ch and data.dtype == np.uint8 and np.array_equal(data, b)
    with wave.open(path) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (ch, 3, 44100, n) and w.readframes(n) == b.tobytes()
    sr2, arr = wavfile.read(path)
    assert sr2 == 44100 and arr.dtype == np.int32 and np.array_equal(arr.reshape(n, ch), v * 256)


def test_read_wav_pcm_extensible_and_other_files(tmp_path):
    from scipy.io import wavfile
    v = np.array([[S.LO, 1], [S.HI, -1], [255, -256]], dtype=np.int32)
    b = audio.pack_s24(v)
    sub = bytes.fromhex("0100000000001000800000aa00389b71")
    fmt = struct.pack("<HHIIHH", 0xFFFE, 2, 48000, 48000 * 6, 6, 24) + struct.pack("<HHI", 22, 24, 3) + sub
    junk = b"LIST" + struct.pack("<I", 3) + b"abc\0"                                            # an odd chunk with its pad byte, in front
    body = b"WAVE" + junk + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", b.size + 2) + b.tobytes() + b"\x11\x22"
    path = str(tmp_path / "ext.wav")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    data, sr, ch = audio.read_wav_pcm(path)                                                     # a trailing partial block is dropped
    assert (sr, ch) == (48000, 2) and np.array_equal(data, b)
    other = fmt[:24] + bytes(16)                                                                 # another sub-format: not ours
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body.replace(fmt, other))
    with pytest.raises(Exception):
        audio.read_wav_pcm(path)                                                                # left to the existing reader, which refuses it
    p16 = str(tmp_path / "p16.wav")
    wavfile.write(p16, 22050, np.arange(-4, 4, dtype=np.int16).reshape(4, 2))
    data, sr, ch = audio.read_wav_pcm(p16)                                                      # everything else: the existing reader's answer
    assert data.dtype == np.int16 and data.shape == (4, 2) and (sr, ch) == (22050, 2)
    for bad in (np.zeros((4, 2), np.uint8), np.zeros((4, 3), np.int16), np.zeros(3, np.uint8)):
        with pytest.raises(ValueError, match="write_wav_s24"):
            audio.write_wav_s24(p16, bad, 8000)


YAML = """
training_config: {{dataset: LJSpeech}}
wave: {{LJSpeech: {{wave_path: 'a.wav', save_pred: 'out'}}}}
mask: {{start_pos_in_sec: 1.0, end_pos_in_sec: 1.2}}
long: {long}
hifi_gan: {{checkpoint_file: 'g/generator_v1'}}
hubert_model: {{type: 'base', LJSpeech: {{model_checkpoint: 'm.pt'}}}}
km_model: {{n_clusters: 100, LJSpeech: {{path2centroids: 'k/', km_model_path: 'k/'}}}}
"""


def test_config_accepts_and_refuses_pcm24(tmp_path):
    from speech_inpainting_amd.config import load_predict_config

    def load(long):
        p = tmp_path / "predict.yaml"
        p.write_text(YAML.format(long=long))
        return load_predict_config(str(p))

    assert load("{rate: file, feed: contexts, pcm24: keep}").long_pcm24 == "keep"
    assert load("{rate: file, feed: contexts, clips16: file, pcm24: keep}").long_pcm24 == "keep"
    assert load("{rate: file, feed: contexts}").long_pcm24 == "float32" and load("{clip_s: 4}").long_pcm24 == "float32"
    assert load("{pcm24: float32}").long_pcm24 == "float32"                                    # the default, anywhere
    with pytest.raises(ValueError, match=r"long.pcm24 = 'drop': float32 \(the default"):
        load("{rate: file, feed: contexts, pcm24: drop}")
    with pytest.raises(ValueError, match=r"long.pcm24 = keep needs `rate: file` and `feed: contexts`"):
        load("{rate: file, pcm24: keep}")
    with pytest.raises(ValueError, match=r"long.pcm24 = keep needs `rate: file` and `feed: contexts`"):
        load("{pcm24: keep}")


def test_engine_shape_refusals_are_host_only():
    """A uint8 input that is not (n, 3) or (n, ch, 3) is refused before the engine looks at its device or weights, and so is
    feed="recording" for a well-formed one."""
    from speech_inpainting_amd.engine import InpaintingEngine
    eng = InpaintingEngine.__new__(InpaintingEngine)                                            # no context: nothing may be launched
    for shape in ((12,), (12, 2), (4, 3, 2), (2, 2, 2, 3), (0,)):
        x = torch.zeros(shape, dtype=torch.uint8)
        for fn in ("find_quiet_runs", "find_dead_runs", "find_gaps"):
            with pytest.raises(ValueError, match=fn + r": a uint8 input is packed 24-bit PCM"):
                getattr(eng, fn)(x)
        with pytest.raises(ValueError, match=r"find_level_runs: a uint8 input is packed 24-bit PCM"):
            eng.find_level_runs(x, half=3)
        with pytest.raises(ValueError, match=r"conceal_file: a uint8 input is packed 24-bit PCM"):
            eng.conceal_file(x, 48000, feed="contexts")
    good = torch.zeros((100, 2, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"conceal_file: packed 24-bit PCM needs feed = 'contexts'"):
        eng.conceal_file(good, 48000)
    with pytest.raises(ValueError, match=r"conceal_file: packed 24-bit PCM at 22050 Hz"):
        eng.conceal_file(good, 22050, feed="contexts")
    assert InpaintingEngine._file_samples(good, "f") == (True, 2) and InpaintingEngine._file_samples(good[:, 0], "f") == (True, 1)
    assert InpaintingEngine._file_samples(torch.zeros(5, 2), "f") == (False, 2)
