"""The library's loader and descriptor check through si_plan_weights / si_pack_weights_host, on the CPU: no device is touched.

Bytes: the packed image equals tests/weights_ref.py's byte for byte from offset 32, for every architecture family, arithmetic and
checkpoint spelling; tests/test_gpu_weights.py shows that the device blob is this image.  Fingerprint, the descriptor table, every
loader refusal, and validation before allocation (a child process under RLIMIT_AS)."""
import ctypes
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from speech_inpainting_amd import native, synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from tests import weights_ref as W
from tests.cases import unit_arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
EINVAL, ENOMEM, EWEIGHTS = -1, -2, -5


@pytest.fixture(autouse=True)
def _default_env(monkeypatch):
    for k in ("SI_VOC_OPREADY", "SI_VOC_RES16"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------------------ checkpoints
def _spell(sd, how):
    """A name -> numpy checkpoint with every weight-normed module in ONE spelling: 'legacy' (weight_g / weight_v), 'param'
    (parametrizations.weight.original0 / 1) or 'folded' (`.weight` = the fp32 fold, which is what the fp32 pack stores)."""
    out = {}
    for k, a in sd.items():
        for g, v in ((".weight_g", ".weight_v"), (".parametrizations.weight.original0", ".parametrizations.weight.original1")):
            if k.endswith(g):
                p = k[:-len(g)]
                if how == "folded":
                    out[p + ".weight"] = W.module_weight(sd, p, 2 if "pos_conv" in p else 0)
                else:
                    out[p + (".weight_g" if how == "legacy" else ".parametrizations.weight.original0")] = a
                break
            if k.endswith(v):
                p = k[:-len(v)]
                if how != "folded":
                    out[p + (".weight_v" if how == "legacy" else ".parametrizations.weight.original1")] = a
                break
        else:
            out[k] = a
    return out


def _state(harch, varch, K=100, seed=5):
    # (a codebook around 0, not around the log-mel level: there `raw = v + centre` differs from the centroid itself in some bits)
    return W.state_arrays(synth.synth_hubert_state(harch, seed), synth.synth_generator_state(varch, seed + 1), synth.synth_codebook(K, harch.codebook_dim, seed + 2) + 5.0)


def _pack(d, sd, slack=64):
    blob, index = W.flatten(sd)
    return native.pack_weights_host(d, blob, index, slack=slack)


def _header(img):
    return dict(magic=int(img[0:4].view(np.uint32)[0]), version=int(img[4:8].view(np.uint32)[0]), fingerprint=int(img[8:16].view(np.uint64)[0]),
                total=int(img[16:24].view(np.uint64)[0]), reserved=int(img[24:32].view(np.uint64)[0]))


LAYER = dict(conv_bias=True, feat_extract_norm="layer", do_stable_layer_norm=True)
PAIRS = {
    "tiny+tiny": (HubertArch.tiny(), VocoderArch.tiny()),
    "layer+v3": (HubertArch.tiny(**LAYER), VocoderArch.v3()),
    "cg48+unit": (HubertArch.tiny(hidden_size=192, num_attention_heads=3, num_conv_pos_embedding_groups=4), unit_arch()),
    "cg64+v3": (HubertArch.tiny(num_conv_pos_embedding_groups=2), VocoderArch.v3()),
}
MATHS = (("fp32", "fp32"), ("bf16", "bf16"), ("fp32", "bf16x3"), ("bf16", "fp16"))
_STATES = {}


def _check_bytes(harch, varch, em, vm, sd, opready=True, res16=True):
    d = native.make_desc(harch, varch, sd["codebook"].shape[0], em, vm)
    ref = W.pack(d, sd, opready, res16)
    rc, total, msg = native.plan_weights(d)
    assert rc == 0 and total == ref["total"], (rc, total, ref["total"], msg)
    images = []
    for how in ("legacy", "param", "folded"):
        rc, img, need, msg = _pack(d, _spell(sd, how))
        assert rc == 0 and need == total, (how, rc, msg)
        h = _header(img)
        assert (h["magic"], h["version"], h["total"], h["reserved"]) == (ref["magic"], ref["version"], total, 0)
        assert (img[need:] == 0xA5).all()                                                  # nothing is written past `needed`
        bad = np.nonzero(img[32:need] != ref["image"])[0]
        assert bad.size == 0, f"{how}: {bad.size} bytes differ from the reference, the first at offset {32 + int(bad[0])}"
        images.append(img)
    assert np.array_equal(images[0], images[1]) and np.array_equal(images[0], images[2])   # header (fingerprint) included
    return ref, images[0]


@pytest.mark.parametrize("em,vm", MATHS)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_image_equals_reference_byte_for_byte(pair, em, vm):
    """Every family: group / layer-norm + conv-bias + stable-layer-norm encoders, posconv groups of 48 and 64 channels, ResBlock1 /
    ResBlock2 generators, the unit vocoder (11 taps at rate 5: absent (phase, tap) pairs; 384 input channels; on the fp16 stream the
    last stage's 16 channels padded to 32); encoder math fp32 / bf16 and vocoder math fp32 / bf16 / bf16x3 / fp16; three spellings."""
    harch, varch = PAIRS[pair]
    sd = _STATES.setdefault(pair, _state(harch, varch))
    ref, _ = _check_bytes(harch, varch, em, vm, sd)
    if pair == "cg48+unit":
        assert ref["layout"].post_C == (32 if vm == "fp16" else 16) and ref["layout"].mel_ld == 384 and ref["layout"].ups[0].ntaps == 3
    if pair == "tiny+tiny":
        assert ref["layout"].mel_ld == 96                                                  # conv_pre's 80 mel channels padded to 96


@pytest.mark.parametrize("env,padded", [({"SI_VOC_RES16": "0"}, False), ({"SI_VOC_OPREADY": "0"}, False), ({"SI_VOC_RES16": "1"}, True)])
def test_unit_vocoder_stage_padding_follows_the_environment(monkeypatch, env, padded):
    harch, varch = PAIRS["cg48+unit"]
    sd = _STATES.setdefault("cg48+unit", _state(harch, varch))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ref, _ = _check_bytes(harch, varch, "bf16", "fp16", sd, opready=env.get("SI_VOC_OPREADY", "1") != "0", res16=env.get("SI_VOC_RES16", "1") != "0")
    assert ref["layout"].post_C == (32 if padded else 16)


def test_benchmark_pair_once():
    """HuBERT-base in bf16 + HiFi-GAN V1 in fp16, the benchmark's pair (its time on the build machine: DESIGN.md 4.23)."""
    harch, varch = HubertArch.base(), VocoderArch.v1()
    sd = _state(harch, varch, K=100, seed=9)
    d = native.make_desc(harch, varch, 100, "bf16", "fp16")
    blob, index = W.flatten(sd)
    t0 = time.perf_counter()
    rc, img, need, msg = native.pack_weights_host(d, blob, index)
    t1 = time.perf_counter()
    ref = W.pack(d, sd)
    print(f"base + V1 (bf16, fp16): {need} bytes, library {t1 - t0:.2f} s, reference {time.perf_counter() - t1:.2f} s")
    assert rc == 0 and need == ref["total"], msg
    assert np.array_equal(img[32:need], ref["image"])


def test_valid_checkpoints_pack_to_the_parent_commits_device_blob():
    """The kernels' operands do not change: for the tiny pair in (bf16, fp16) the host image equals the device blob the commit before
    the host entry existed produced on an MI355X from the same checkpoint (its SHA-256, recorded then: DESIGN.md 4.23)."""
    from speech_inpainting_amd.checkpoint import flatten_checkpoint
    harch, varch = HubertArch.tiny(), VocoderArch.tiny()
    blob, index = flatten_checkpoint(synth.synth_hubert_state(harch), synth.synth_generator_state(varch), synth.synth_codebook(100, 80))
    rc, img, need, msg = native.pack_weights_host(native.make_desc(harch, varch, 100, "bf16", "fp16"), blob, index)
    assert rc == 0, msg
    assert (need, hashlib.sha256(img.tobytes()).hexdigest()) == PARENT_BLOB


PARENT_BLOB = (8232192, "09bbe432f16534c3d80b1d6cf4769ed9501ab84b36da56ca2c3fe2cf9bb95f3d")


# ------------------------------------------------------------------------------------------------------------ fingerprint
def test_fingerprint(monkeypatch):
    harch, varch = PAIRS["cg48+unit"]
    sd = _STATES.setdefault("cg48+unit", _state(harch, varch))

    def fp(d, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rc, img, need, msg = _pack(d, sd)
        for k in env:
            monkeypatch.delenv(k)
        assert rc == 0, msg
        return _header(img)["fingerprint"], need

    d = native.make_desc(harch, varch, 100, "bf16", "fp16")
    base = fp(d)
    assert base == fp(native.make_desc(harch, varch, 100, "bf16", "fp16")) and base == fp(d, SI_VOC_RES16="1", SI_VOC_OPREADY="1")
    assert fp(d, SI_VOC_RES16="0")[0] != base[0] and fp(d, SI_VOC_OPREADY="0")[0] != base[0]         # the last stage is 16 wide, not 32
    for em, vm in (("fp32", "fp16"), ("bf16", "bf16"), ("bf16", "bf16x3")):
        assert fp(native.make_desc(harch, varch, 100, em, vm))[0] != base[0]
    # a field that moves bytes without moving the total: the resblock flavour only renames tensors here, the chunk is arithmetic-free
    d2 = native.make_desc(harch, varch, 100, "bf16", "fp16", vocoder_chunk=4)
    assert fp(d2)[1] == base[1] and fp(d2)[0] != base[0]
    # options that move no stage width leave it alone: fp32 keeps the real widths whatever SI_VOC_RES16 says
    d3 = native.make_desc(harch, varch, 100, "bf16", "fp32")
    assert fp(d3) == fp(d3, SI_VOC_RES16="0")


# ------------------------------------------------------------------------------------------------------------ descriptor table
def _desc():
    return native.make_desc(HubertArch.tiny(), VocoderArch.tiny(), 100, "fp32", "fp32")


def _refused(d, field):
    rc, total, msg = native.plan_weights(d)
    assert rc == EINVAL and total == 0, (field, rc, total, msg)
    assert field in msg, (field, msg)
    return msg


SCALARS = {"struct_size": 1, "hidden_size": 64, "num_layers": 1, "num_heads": 1, "intermediate_size": 16, "num_conv": 1, "pos_conv_kernel": 1,
           "pos_conv_groups": 1, "codebook_dim": 1, "num_clusters": 1, "num_mels": 1, "num_ups": 1, "up_initial_channel": 32, "num_rb": 1,
           "num_dil": 1, "encoder_math": 1, "vocoder_math": 1, "resblock_type": 1}
LEGAL = {("encoder_math", 0), ("vocoder_math", 0), ("resblock_type", 0)}
ANY_VALUE = ("conv_bias", "feat_norm_layer", "stable_layer_norm", "feat_proj_layer_norm", "vocoder_chunk")


def _values(align):
    return sorted({0, -1, -align, INT_MAX})


def test_descriptor_table_scalars():
    assert set(SCALARS) | set(ANY_VALUE) | {"conv_dim", "conv_kernel", "conv_stride", "layer_norm_eps", "up_rates", "up_kernels", "rb_kernels",
                                            "rb_dilations"} == {f[0] for f in native.ModelDesc._fields_}
    assert native.plan_weights(_desc())[0] == 0
    for field, align in SCALARS.items():
        for v in _values(align):
            if (field, v) in LEGAL:
                continue
            d = _desc()
            setattr(d, field, v)
            _refused(d, field)
    for field in ANY_VALUE:                                        # flags are read as booleans, a chunk <= 0 means the default
        for v in (0, -1, 1, INT_MAX):
            d = _desc()
            setattr(d, field, v)
            assert native.plan_weights(d)[0] == 0, (field, v)
    for eps in (float("nan"), float("inf"), -float("inf"), -1.0, 0.0, -0.0):
        d = _desc()
        d.layer_norm_eps = eps
        _refused(d, "layer_norm_eps")


def test_descriptor_table_used_array_elements():
    d0 = _desc()
    arrays = [("conv_dim", 16, d0.num_conv), ("conv_kernel", 1, d0.num_conv), ("conv_stride", 1, d0.num_conv), ("up_rates", 1, d0.num_ups),
              ("up_kernels", 1, d0.num_ups), ("rb_kernels", 1, d0.num_rb)]
    for field, align, n in arrays:
        for i in range(n):
            for v in _values(align):
                d = _desc()
                getattr(d, field)[i] = v
                _refused(d, f"{field}[{i}]")
        if n < len(getattr(d0, field)):                             # an UNUSED element may hold anything
            d = _desc()
            getattr(d, field)[n] = -7
            assert native.plan_weights(d)[0] == 0, field
    for j in range(d0.num_rb):
        for n in range(d0.num_dil):
            for v in _values(1):
                d = _desc()
                d.rb_dilations[j][n] = v
                _refused(d, f"rb_dilations[{j}][{n}]")
    d = _desc()
    d.rb_dilations[3][3] = -7
    assert native.plan_weights(d)[0] == 0


def test_the_probed_descriptors_are_refused():
    """The 19 descriptors a probe of the earlier check found accepted, one of them a division by zero in the planner."""
    def mk(**kw):
        d = _desc()
        for k, v in kw.items():
            if isinstance(k, str) and "@" in k:
                name, idx = k.split("@")
                a = getattr(d, name)
                for i in idx.split("_")[:-1]:
                    a = a[int(i)]
                a[int(idx.split("_")[-1])] = v
            else:
                setattr(d, k, v)
        return d
    probes = [("num_layers", mk(num_layers=-1)), ("intermediate_size", mk(intermediate_size=0)), ("intermediate_size", mk(intermediate_size=-16)),
              ("conv_dim[3]", mk(**{"conv_dim@3": 0})), ("conv_dim[3]", mk(**{"conv_dim@3": -16})), ("num_mels", mk(num_mels=0)), ("num_mels", mk(num_mels=-5)),
              ("pos_conv_kernel", mk(pos_conv_kernel=0)), ("pos_conv_kernel", mk(pos_conv_kernel=-1)), ("up_initial_channel", mk(up_initial_channel=0)),
              ("up_initial_channel", mk(up_initial_channel=-512)), ("rb_kernels[1]", mk(**{"rb_kernels@1": -1})), ("rb_dilations[0][0]", mk(**{"rb_dilations@0_0": 0})),
              ("layer_norm_eps", mk(layer_norm_eps=float("nan"))), ("layer_norm_eps", mk(layer_norm_eps=-1.0)),
              ("up_rates[2]", mk(**{"up_rates@2": -2, "up_kernels@2": 0})), ("num_clusters", mk(num_clusters=INT_MAX)),
              ("up_rates[1]", mk(**{"up_rates@1": 0, "up_kernels@1": 0})), ("up_rates[0]", mk(**{"up_rates@0": 0, "up_kernels@0": 0}))]
    assert len(probes) == 19
    for field, d in probes:
        _refused(d, field)


def test_widths_a_kernel_of_the_first_forward_refuses_are_refused_at_load():
    """Descriptors inside every range that conv0_check, si_launch_layernorm or si_launch_conv_post would refuse in the first pass: each
    names its field; the neighbour on the accepted side of each rule plans."""
    def enc(**kw):
        return native.make_desc(HubertArch.tiny(**kw), VocoderArch.tiny(), 100, "fp32", "fp32")

    def gen(**kw):
        return native.make_desc(HubertArch.tiny(), VocoderArch(**kw), 100, "fp32", "fp16")
    k7 = (10, 3, 3, 3, 3, 2, 2)
    wide = dict(hidden_size=2112, num_attention_heads=33)
    one = dict(upsample_rates=(1,), upsample_kernel_sizes=(3,))
    refused = [("conv_kernel[0]", enc(conv_kernel=(8,) + k7[1:])), ("conv_kernel[0]", enc(conv_kernel=(11,) + k7[1:])),
               ("conv_dim[0]", enc(conv_dim=(48,) + (32,) * 6)), ("conv_dim[0]", enc(conv_dim=(2048,) + (32,) * 6)),
               ("conv_dim[0]", enc(conv_dim=(1040,) + (32,) * 6, feat_extract_norm="layer")),
               ("hidden_size", enc(**wide)), ("hidden_size", enc(do_stable_layer_norm=True, **wide)),
               ("conv_dim[3]", enc(conv_dim=(32, 32, 32, 2064, 32, 32, 32), feat_extract_norm="layer")),
               ("conv_dim[6]", enc(conv_dim=(32,) * 6 + (2064,))),
               ("final generator width 256", gen(upsample_initial_channel=512, **one)),
               ("final generator width 160", gen(upsample_initial_channel=320, **one))]
    for field, d in refused:
        _refused(d, field)
    accepted = [enc(conv_dim=(1024,) + (32,) * 6), enc(conv_dim=(16,) + (32,) * 6), enc(hidden_size=2048, num_attention_heads=32),
                enc(conv_dim=(32, 32, 32, 2048, 32, 32, 32), feat_extract_norm="layer"),
                enc(conv_dim=(32, 32, 32, 2064, 32, 32, 32)),                       # group flavour: only the last width is LayerNormed
                enc(conv_dim=(32,) * 6 + (2064,), feat_proj_layer_norm=False), enc(conv_dim=(32,) * 6 + (2048,)),
                gen(upsample_initial_channel=288, **one),                           # 144 wide at the end: the widest multiple of 16 under 148
                gen(num_mels=1, upsample_initial_channel=64, **one), gen(num_mels=81, upsample_initial_channel=64, **one)]                  # conv_pre's rows are padded to 32 / 96 channels
    for d in accepted:
        rc, total, msg = native.plan_weights(d)
        assert rc == 0 and total > 0, msg


def test_bounds_leave_the_real_models_a_wide_margin():
    for harch, varch, K in ((HubertArch.base(), VocoderArch.v1(), 100), (HubertArch.large(), VocoderArch.v1(), 500), (HubertArch.base(), VocoderArch.v3(), 100),
                            (HubertArch.large(), unit_arch(), 500)):
        d = native.make_desc(harch, varch, K, "bf16", "fp16")
        rc, total, msg = native.plan_weights(d)
        assert rc == 0 and 0 < total < 2 ** 32, msg
        # (hidden_size: twice HuBERT-large is the widest LayerNorm row, SI_LN_MAX_WIDTH; beyond it the first forward used to fail)
        for field, factor in (("hidden_size", 2), ("intermediate_size", 4), ("num_layers", 2), ("num_clusters", 100), ("up_initial_channel", 4), ("num_mels", 8)):
            d = native.make_desc(harch, varch, K, "bf16", "fp16")
            setattr(d, field, getattr(d, field) * factor)
            if field == "hidden_size":
                d.num_heads *= factor
            assert native.plan_weights(d)[0] == 0, (field, factor)


# ------------------------------------------------------------------------------------------------------------ loader refusals
MICRO_H = HubertArch.tiny(num_hidden_layers=1, intermediate_size=128)
MICRO_V = VocoderArch(upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=64, resblock_kernel_sizes=(3,),
                      resblock_dilation_sizes=((1,),))


def _micro(vm="fp32"):
    sd = _STATES.setdefault("micro", _state(MICRO_H, MICRO_V, K=10))
    return native.make_desc(MICRO_H, MICRO_V, 10, "fp32", vm), dict(sd)


def _refused_load(d, blob, index, *names):
    rc, img, need, msg = native.pack_weights_host(d, blob, index, slack=64)
    assert rc == EWEIGHTS, (rc, msg, names)
    assert need == native.plan_weights(d)[1]
    assert (img == 0xA5).all(), "a refused load wrote into the output"
    for n in names:
        assert n in msg, (n, msg)
    return msg


def test_malformed_indexes_are_refused_by_line_or_name():
    d, sd = _micro()
    blob, index = W.flatten(sd)
    assert native.pack_weights_host(d, blob, index)[0] == 0
    first = index.split("\n")[0].split()[0]
    _refused_load(d, blob, "", "empty")
    _refused_load(d, blob, "\n\n", "empty")
    _refused_load(d, blob, index + "foo bar\n", "line", "foo bar")
    _refused_load(d, blob, index + "x 0 9 1 1 1 1 1 1 1 1 1\n", "line", "malformed")                 # nd > 8
    _refused_load(d, blob, index + "x 0 -1\n", "line", "malformed")
    _refused_load(d, blob, index + "x 0 2 4 -3\n", "line", "x")                                       # negative dim
    _refused_load(d, blob, index + "x 0 2 4\n", "line", "x")                                          # fewer dims than announced
    _refused_load(d, blob, index + "x 0 2 3037000500 3037000500\n", "x", "overflow")                  # the product overflows a signed 64-bit count
    _refused_load(d, blob, index + "x 0 3 4294967296 4294967296 4\n", "x", "overflow")                # ... and an unsigned one
    _refused_load(d, blob, index + "x 0 2 2147483648 2147483648\n", "x")                              # 2^62 floats: the byte count overflows
    _refused_load(d, blob, index + "x -4 1 1\n", "x", "offset -4")
    _refused_load(d, blob, index + "x 2 1 1\n", "x", "offset 2")                                      # misaligned
    _refused_load(d, blob, index + f"x {blob.nbytes} 1 1\n", "x", "does not fit")                     # past the blob
    _refused_load(d, blob, index + f"x {blob.nbytes - 4} 1 2\n", "x", "does not fit")
    _refused_load(d, blob, index + f"x {2 ** 63 - 4} 1 1\n", "x", "does not fit")
    _refused_load(d, blob, index + index.split("\n")[0] + "\n", first, "twice")                       # a duplicate name
    rc, _, _, msg = native.pack_weights_host(d, blob, index + f"spare {blob.nbytes - 4} 1 1\nempty {blob.nbytes} 1 0\n")
    assert rc == 0, msg                                                                                 # extra tensors are ignored


def test_every_required_tensor_missing_or_misshaped():
    d, sd = _micro()
    req = W.required(d)
    assert len(req) > 50
    for item in req:
        if item[0] == "tensor":
            name = item[1]
            gone = {k: v for k, v in sd.items() if k != name}
            _refused_load(d, *W.flatten(gone), name, "missing")
            bad = dict(sd)
            bad[name] = sd[name].reshape(sd[name].shape + (1,))
            _refused_load(d, *W.flatten(bad), name, "shape")
        else:
            prefix = item[1]
            keys = [k for k in sd if k.startswith(prefix + ".weight") or k.startswith(prefix + ".parametrizations.")]
            assert len(keys) == 2
            gone = {k: v for k, v in sd.items() if k not in keys}
            _refused_load(d, *W.flatten(gone), prefix, "neither")
            vkey = [k for k in keys if k.endswith("_v") or k.endswith("original1")][0]
            gkey = [k for k in keys if k != vkey][0]
            gone = {k: v for k, v in sd.items() if k != vkey}
            _refused_load(d, *W.flatten(gone), vkey, "missing")
            bad = dict(sd)
            bad[vkey] = np.ascontiguousarray(sd[vkey].transpose(0, 2, 1)) if sd[vkey].shape[1] != sd[vkey].shape[2] else sd[vkey][:, :, :-1].copy()
            _refused_load(d, *W.flatten(bad), vkey, "shape")
            bad = dict(sd)
            bad[gkey] = np.concatenate([sd[gkey].reshape(-1), np.ones(1, np.float32)])
            _refused_load(d, *W.flatten(bad), gkey, "magnitudes")
            folded = _spell(sd, "folded")
            bad = dict(folded)
            bad[prefix + ".weight"] = folded[prefix + ".weight"].reshape(-1)
            _refused_load(d, *W.flatten(bad), prefix + ".weight", "shape")


def test_non_finite_values_and_zero_norm_rows_are_refused():
    d, sd = _micro()
    used = {(i[1] if i[0] == "tensor" else None) for i in W.required(d)}
    for name, a in sd.items():
        module = any(name.endswith(s) for s in ("weight_g", "weight_v", "original0", "original1"))
        assert module or name in used, name
        for k, bad_value in enumerate((np.nan, np.inf, -np.inf)):
            if k and a.size > 4096:
                continue
            bad = dict(sd)
            b = a.copy().reshape(-1)
            b[(7 * (k + 1)) % b.size] = bad_value
            bad[name] = b.reshape(a.shape)
            _refused_load(d, *W.flatten(bad), name, "non-finite")
    # finite magnitudes whose fold overflows: g / ||v|| = inf
    bad = dict(sd)
    g = sd["generator.conv_pre.weight_g"].copy()
    g.reshape(-1)[3] = 3e38
    bad["generator.conv_pre.weight_g"] = g
    bad["generator.conv_pre.weight_v"] = sd["generator.conv_pre.weight_v"] * np.float32(1e-3)
    _refused_load(d, *W.flatten(bad), "generator.conv_pre", "non-finite")
    # a finite codebook whose fp32 column sum overflows
    bad = dict(sd)
    bad["codebook"] = np.full_like(sd["codebook"], 3e38)
    _refused_load(d, *W.flatten(bad), "codebook", "non-finite")
    # zero-norm rows: dim 0 of a generator module, dim 2 of the positional conv
    for name, sl in (("generator.ups.1.weight_v", (5,)), ("generator.conv_post.weight_v", (0,)),
                     ("base_model.encoder.pos_conv_embed.conv.parametrizations.weight.original1", (slice(None), slice(None), 9))):
        bad = dict(sd)
        v = sd[name].copy()
        v[sl] = 0.0
        bad[name] = v
        msg = _refused_load(d, *W.flatten(bad), name, "zero norm")
        assert f"row {sl[-1]}" in msg
    # ... while a zero row of a module that comes folded is simply a zero row
    folded = _spell(sd, "folded")
    folded["generator.ups.1.weight"] = folded["generator.ups.1.weight"].copy()
    folded["generator.ups.1.weight"][5] = 0.0
    assert _pack(d, folded)[0] == 0


def test_fp16_saturation_of_a_finite_weight_stays_a_silent_clamp():
    d, sd = _micro("fp16")
    sd = _spell(sd, "folded")
    w = sd["generator.conv_pre.weight"].copy()
    w[3, 2, 1], w[4, 2, 1] = 1e5, -70000.0
    sd["generator.conv_pre.weight"] = w
    rc, img, need, msg = _pack(d, sd)
    assert rc == 0, msg
    ref = W.pack(d, sd)
    assert np.array_equal(img[32:need], ref["image"])
    G = ref["layout"].pre
    words = img[G.w:G.w + 2 * G.ntaps * G.Npad * G.Cin].view(np.uint16).reshape(G.ntaps, G.Npad, G.Cin)
    assert words[1, 3, 2] == 0x7BFF and words[1, 4, 2] == 0xFBFF


def test_capacity_and_null_arguments():
    d, sd = _micro()
    blob, index = W.flatten(sd)
    total = native.plan_weights(d)[1]
    rc, img, need, msg = native.pack_weights_host(d, blob, index, capacity=total - 1, slack=1)
    assert rc == ENOMEM and need == total and (img == 0xA5).all() and str(total) in msg
    lib = native.load_library()
    need = ctypes.c_size_t(0)
    assert lib.si_pack_weights_host(ctypes.byref(d), None, 0, index.encode(), None, 0, ctypes.byref(need), None, 0) == EINVAL
    assert lib.si_plan_weights(ctypes.byref(d), None) == EINVAL and lib.si_plan_weights(None, ctypes.byref(need)) == EINVAL
    bad = _desc()
    bad.num_mels = 0
    rc, img, need, msg = native.pack_weights_host(bad, blob, index, capacity=64)
    assert rc == EINVAL and need == 0 and "num_mels" in msg and (img == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------ validate before allocating
_CHILD = r"""
import ctypes, os, resource, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from speech_inpainting_amd import native, synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from tests import weights_ref as W
harch = HubertArch.tiny(num_hidden_layers=1, intermediate_size=128)
varch = VocoderArch(upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=64, resblock_kernel_sizes=(3,), resblock_dilation_sizes=((1,),))
K = 65536                                                         # a valid desc whose plan is dominated by 2 x 21 MB of codebook tables
sd = W.state_arrays(synth.synth_hubert_state(harch, 5), synth.synth_generator_state(varch, 6), synth.synth_codebook(K, 80, 7))
d = native.make_desc(harch, varch, K, "fp32", "fp32")
rc, total, msg = native.plan_weights(d)
assert rc == 0 and total > 40 << 20, (rc, total, msg)
blob, index = W.flatten(sd)
short = "\n".join(l for l in index.split("\n") if not l.startswith("generator.conv_post.bias")) + "\n"
out = np.full(total, 0xA5, np.uint8)                               # the caller's buffer exists before the limit drops
lib = native.load_library()
vm = [int(l.split()[1]) * 1024 for l in open("/proc/self/status") if l.startswith("VmSize")][0]
hard = resource.getrlimit(resource.RLIMIT_AS)[1]
resource.setrlimit(resource.RLIMIT_AS, (vm + (16 << 20), hard))                   # less room than the image needs, enough for the index
def call(ix):
    need, err = ctypes.c_size_t(0), ctypes.create_string_buffer(512)
    rc = lib.si_pack_weights_host(ctypes.byref(d), blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, ix.encode(), out.ctypes.data_as(ctypes.c_void_p),
                                  total, ctypes.byref(need), err, 512)
    return rc, err.value.decode()
rc1, m1 = call(short)          # a tensor is missing: found BEFORE the image is allocated, so the answer is about the tensor
rc2, m2 = call(index)          # nothing is missing: the allocation fails, as an error code and not as an exception through the C ABI
resource.setrlimit(resource.RLIMIT_AS, (hard, hard))
print("RESULT", rc1, "|", m1, "|", rc2, "|", m2)
assert (out == 0xA5).all()
"""


def test_validates_before_allocating_and_no_exception_leaves_the_abi():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    line = [l for l in r.stdout.split("\n") if l.startswith("RESULT")][0]
    rc1, m1, rc2, m2 = [s.strip() for s in line[len("RESULT"):].split("|")]
    assert int(rc1) == EWEIGHTS and "generator.conv_post.bias" in m1 and "missing" in m1, line
    assert int(rc2) == ENOMEM and "allocate" in m2, line
