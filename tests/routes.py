"""The smallest shapes that reach each route of the three passes, shared by the tests that run every route: the engines,
the encoder's, the generator's and the mel front-end's entry points.  A switch in `env` is set while the engine's context is created;
engines are kept for the session under a key that holds the switches.
A plain module, imported by name: it registers no fixture and no plugin, and importing it needs no GPU."""
import dataclasses

import torch

from tests import cases
from tests.harness import build_engine


def _tail(x, lens, value, dim=-1):
    """A copy of x with everything at and past lens[b] along `dim` of row b set to `value`."""
    y = x.clone()
    for b, n in enumerate(lens):
        y[b].narrow(dim if dim < 0 else dim - 1, int(n), y.shape[dim] - int(n)).fill_(value)
    return y


def _i32(v):
    return torch.tensor([int(a) for a in v], dtype=torch.int32).cuda()


# ------------------------------------------------------------------------------------------------------------ encoder
def _tiny():
    from speech_inpainting_amd.arch import HubertArch
    return HubertArch.tiny()


def _base():
    from speech_inpainting_amd.arch import HubertArch
    return HubertArch(num_hidden_layers=1)


def _large():
    from speech_inpainting_amd.arch import HubertArch
    return dataclasses.replace(HubertArch.large(), num_hidden_layers=1)


def _enc_engine(harch, math, env=None):
    from speech_inpainting_amd.arch import VocoderArch
    key = ("test_gpu_scratch", "enc", harch.hidden_size, harch.feat_extract_norm, math, tuple(sorted((env or {}).items())))
    return build_engine(harch, VocoderArch.tiny(), 50, math, "fp32", env=env, state=(cases._enc_state(harch), None, None), key=key)


def _forward_plain(eng, wave, ms, ml):
    """si_hubert_forward itself (engine.encode goes through si_hubert_forward_padded with valid_len = NULL)."""
    from speech_inpainting_amd.native import _ptr
    return eng.ctx._encoder_call("si_hubert_forward", wave, eng.ctx.desc.codebook_dim, (ms, ml), lambda _: (_ptr(ms), _ptr(ml), 1))


def _encoder_entries(eng, harch, B, N, seed, only=None):
    """{entry point: run} on a batch of B clips of N samples: uniform, padded, ragged (one clip at the receptive field's minimum -- one
    frame -- and one that fills its row), one span table (uniform and ragged), extract_features."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.native import SpanTable
    wave = synth.synth_wave(B, N, seed).cuda()
    T = harch.num_frames(N)
    ms, ml = _i32([320 * (2 + b) + 80 for b in range(B)]), _i32([320 * 3 - 81] * B)
    lens = ([N, 400, (N * 5 // 9) | 1] + [N] * B)[:B]
    assert harch.num_frames(400) == 1 and harch.num_frames(399) == 0 and max(lens) == N
    valid = _i32(lens)
    spans = [[(800 + 37 * b, 700), (N // 2, 333 + b)] for b in range(B)]
    spans[1] = [(0, 100), (250, 4000)]                    # the one-frame clip: a span from sample 0 and one that leaves the clip
    tab = SpanTable(spans, eng.device)
    add = torch.full((B,), 1e-6, dtype=torch.float64).cuda()
    entries = {
        "forward": lambda: _forward_plain(eng, wave, ms, ml),
        "padded": lambda: eng.encode(wave, ms, ml, valid_len=valid),
        "varlen": lambda: eng.encode_ragged(wave, lens, ms, ml),
        "spans": lambda: eng.encode(wave, spans=tab),
        "spans_ragged": lambda: eng.encode_ragged(wave, lens, spans=tab),
        "extract": lambda: eng.extract_features(wave, 1, "layer_norm", ms, ml, add),
    }
    assert T >= 8
    return {k: v for k, v in entries.items() if only is None or k in only}, wave, lens, (ms, ml, tab)


# ------------------------------------------------------------------------------------------------------------ generator
def _varch(name):
    from speech_inpainting_amd.arch import VocoderArch
    return {"v1": VocoderArch.v1, "v3": VocoderArch.v3, "unit": cases.unit_arch}[name]()


VOC_CONFIGS = [("v1", "fp16", {}), ("v1", "fp32", {}), ("v1", "bf16x3", {}), ("v1", "bf16", {}), ("v1", "fp16", {"SI_VOC_CHAIN": "0"}),
               ("v1", "fp16", {"SI_VOC_FUSE": "0"}), ("v3", "fp16", {}), ("unit", "fp16", {})]
VOC_TM, VOC_RAGGED = (1, 57, 130), [57, 1, 30]


def _voc_engine(arch, math, env, chunk=0):
    varch = _varch(arch)
    key = ("test_gpu_scratch", "voc", arch, math, tuple(sorted(env.items())), chunk)
    return build_engine(_tiny(), varch, 50, "fp32", math, vocoder_chunk=chunk, env=env, state=(None, cases._state(varch), None), key=key), varch


def _voc_id(c):
    return "-".join([c[0], c[1]] + [f"{k}={v}" for k, v in c[2].items()])


def _uniform_mel(varch, Tm):
    """The B = 3 batch of Tm frames the generator routes run on."""
    return cases._mel(3, Tm, 300 + Tm, varch.num_mels).cuda()


def _ragged_mel(varch):
    """The B = 3 batch whose clips hold VOC_RAGGED frames of max(VOC_RAGGED)."""
    return cases._mel(3, max(VOC_RAGGED), 400, varch.num_mels).cuda()


# ------------------------------------------------------------------------------------------------------------ mel front-end
def _mel_engine(env=None):
    from speech_inpainting_amd.arch import VocoderArch
    return build_engine(_tiny(), VocoderArch.tiny(), 50, env=env, key=("test_gpu_scratch", "mel", tuple(sorted((env or {}).items()))))


MEL_N22 = (22064, 22063)


def _mel_entries(eng, N22):
    """B = 3 clips of N22 samples; the ragged batch holds one clip at the shortest length si_mel_frames accepts (400 samples: one
    frame) and one that fills its row -> ([run] on the uniform batch, {name: run(wave)} of the ragged entry points, wave, lens)."""
    from speech_inpainting_amd import synth
    from speech_inpainting_amd.native import SpanTable
    ctx = eng.ctx
    assert ctx.mel_frames(400) == 1 and ctx.mel_frames(399) == 0
    wave = synth.synth_wave(3, N22, 21, sr=22050).cuda()
    lens = [N22, 400, 9999]
    s, e = _i32([3000, 50, 4000]), _i32([5205, 300, 6205])
    tab = SpanTable([[(3000, 2205), (9000, 100)], [(0, 60), (390, 500)], []], eng.device)
    uniform = [lambda: eng.mel(wave, s, e), lambda: eng.mel(wave), lambda: eng.mel(wave, spans=tab), lambda: eng.get_mel(wave)]
    ragged = {"varlen": lambda w: eng.mel_ragged(w, lens, s, e), "spans": lambda w: eng.mel_ragged(w, lens, spans=tab)}
    return uniform, ragged, wave, lens
