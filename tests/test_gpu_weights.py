"""The device side of the weight loader, on the tiny architectures: the device blob IS the host image of si_pack_weights_host
(which tests/test_weights_host.py pins byte for byte on the CPU), a refused load changes nothing, a second load replaces the
first completely, the header is checked, and what the source checkpoint held travels with the blob."""
import numpy as np
import pytest
import torch

from speech_inpainting_amd import native, synth
from speech_inpainting_amd.arch import HubertArch, VocoderArch
from speech_inpainting_amd.checkpoint import flatten_checkpoint
from tests.common import case_engine, load_case, run_case

pytestmark = pytest.mark.gpu

HARCH, VARCH, K = HubertArch.tiny(), VocoderArch.tiny(), 100


def _ckpt(seed=5, folded=False):
    return flatten_checkpoint(synth.synth_hubert_state(HARCH, seed), synth.synth_generator_state(VARCH, seed + 1, folded=folded),
                              synth.synth_codebook(K, 80, seed + 2))


def _ctx(enc, voc):
    return native.NativeContext(native.make_desc(HARCH, VARCH, K, enc, voc), torch.device("cuda:0"))


def _host_image(enc, voc, blob, index):
    rc, img, need, msg = native.pack_weights_host(native.make_desc(HARCH, VARCH, K, enc, voc), blob, index)
    assert rc == 0 and need == img.size, msg
    return img


def _dev_bytes(ctx):
    return ctx.weights_tensor().cpu().numpy().copy()


@pytest.mark.parametrize("enc,voc", [("fp32", "fp32"), ("bf16", "fp16"), ("bf16", "bf16x3")])
def test_device_blob_equals_host_image(enc, voc):
    """After load_weights the device blob equals si_pack_weights_host's image byte for byte, header included: what the CPU tests
    say about the image they say about the kernels' operands."""
    blob, index = _ckpt()
    ctx = _ctx(enc, voc)
    ctx.load_weights(blob, index)
    got, want = _dev_bytes(ctx), _host_image(enc, voc, blob, index)
    assert got.size == want.size == ctx.weights_ptr()[1]
    assert np.array_equal(got, want)
    ctx.weights_check()
    ctx.close()


def test_refused_load_changes_nothing():
    c = load_case("tiny_group")
    eng = case_engine(c, "bf16", "fp16")
    before_bytes, before = _dev_bytes(eng.ctx), run_case(eng, c)
    hsd, gsd, cb = c["hsd"], c["gsd"], c["cb"]
    blob, index = flatten_checkpoint(hsd, gsd, cb)
    missing = "\n".join(l for l in index.split("\n") if not l.startswith("generator.ups.1.bias")) + "\n"
    nan = blob.copy()
    nan[blob.size // 2] = np.nan
    for what, (b, ix) in {"missing": (blob, missing), "non-finite": (nan, index), "malformed": (blob, index + "oops 12\n")}.items():
        with pytest.raises(native.NativeError, match=r"\(-5\).*" + what):
            eng.ctx.load_weights(b, ix)
        assert np.array_equal(_dev_bytes(eng.ctx), before_bytes), what
    after = run_case(eng, c)
    assert all(torch.equal(before[k], after[k]) for k in before) and set(before) == set(after)
    eng.ctx.close()


def test_second_load_replaces_the_first():
    """Other weights: the bits of a fresh context.  And nothing of the first load survives in the padding: the device blob is
    filled with 0xFF in between, the second checkpoint is the smaller, folded spelling, and every byte equals the host image."""
    first, second = _ckpt(5), _ckpt(21, folded=True)
    assert second[0].size < first[0].size
    ctx = _ctx("bf16", "fp16")
    ctx.load_weights(*first)
    ctx.weights_tensor().fill_(0xFF)
    ctx.load_weights(*second)
    fresh = _ctx("bf16", "fp16")
    fresh.load_weights(*second)
    got = _dev_bytes(ctx)
    assert np.array_equal(got, _dev_bytes(fresh)) and np.array_equal(got, _host_image("bf16", "fp16", *second))
    wave = synth.synth_wave(2, 8000, 3).cuda()
    a, b = ctx.hubert_forward(wave, None, None), fresh.hubert_forward(wave, None, None)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert not np.array_equal(got, _host_image("bf16", "fp16", *first))
    ctx.close(); fresh.close()


def test_header_is_checked():
    """One flipped byte of the fingerprint in a received blob: si_weights_check and the first forward both answer SI_EWEIGHTS; the
    reserved word is not part of the check."""
    blob, index = _ckpt()
    src, dst = _ctx("bf16", "fp16"), _ctx("bf16", "fp16")
    src.load_weights(blob, index)
    dst.alloc_weights()
    w = dst.weights_tensor()
    w.copy_(src.weights_tensor())
    w[24:32] = 0x5A                                                 # the reserved word may hold anything
    dst.weights_check()
    dst.alloc_weights()                                             # a receiving rank again: not yet verified
    w[9] ^= 0x10
    wave = synth.synth_wave(1, 8000, 3).cuda()
    with pytest.raises(native.NativeError, match=r"si_weights_check failed \(-5\)"):
        dst.weights_check()
    with pytest.raises(native.NativeError, match=r"\(-5\).*different layout"):
        dst.hubert_forward(wave, None, None)
    w[9] ^= 0x10
    a, b = dst.hubert_forward(wave, None, None), src.hubert_forward(wave, None, None)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    del w
    src.close(); dst.close()
