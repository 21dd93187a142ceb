"""tests/poison.py on the CPU: the fill patterns read as DESIGN.md 4.22 says, poisoned_allocs poisons and restores, and every
launcher of csrc/*.hip is in exactly one of the two family lists."""
import glob
import math
import os
import re

import pytest
import torch

from tests import poison as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fill_bytes_read_as_the_table_says():
    assert P.FILLS == (0x00, 0xFF, 0x7B)
    for dt in (torch.float32, torch.float16, torch.bfloat16, torch.int32):
        assert float(P.fill_value(0x00, dt)) == 0.0
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert math.isnan(float(P.fill_value(0xFF, dt))), dt
    assert int(P.fill_value(0xFF, torch.int32)) == -1
    f32, f16, bf16 = (float(P.fill_value(0x7B, dt)) for dt in (torch.float32, torch.float16, torch.bfloat16))
    assert f16 == 61280.0                                   # 0x7B7B: 2^15 * (1 + 891 / 1024)
    assert math.isfinite(f32) and 1.30e36 < f32 < 1.31e36   # 0x7B7B7B7B
    assert math.isfinite(bf16) and 1.30e36 < bf16 < 1.31e36 and bf16 <= f32
    assert int(P.fill_value(0x7B, torch.int32)) == 0x7B7B7B7B > 2 ** 30


def _settings():
    return (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
            torch.utils.deterministic.fill_uninitialized_memory)


def test_poisoned_allocs_poisons_torch_empty_and_restores_both_settings():
    before = _settings()
    with P.poisoned_allocs():
        assert bool(torch.isnan(torch.empty(1000, dtype=torch.float32)).all())
        assert bool((torch.empty(1000, dtype=torch.uint8) == 255).all())
        assert bool((torch.empty(1000, dtype=torch.int32) == 2 ** 31 - 1).all())
        assert bool((torch.empty(1000, dtype=torch.int64) == 2 ** 63 - 1).all())
        assert bool((torch.empty(1000, dtype=torch.int16) == 32767).all())
    assert _settings() == before
    with pytest.raises(KeyError):
        with P.poisoned_allocs():
            raise KeyError("the body raises")
    assert _settings() == before
    # and from the other starting point
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = False
    try:
        inside = _settings()
        with P.poisoned_allocs():
            assert torch.utils.deterministic.fill_uninitialized_memory is True
        assert _settings() == inside
    finally:
        torch.utils.deterministic.fill_uninitialized_memory = before[2]
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])
    assert _settings() == before


class _FakeCtx:
    """What poison_scratch asks of a context: the three workspace attributes (here host tensors, one of them absent)."""
    def __init__(self, n):
        self._ws = torch.zeros(4 * n, dtype=torch.uint8)
        self._ws_mel = torch.zeros(4 * n, dtype=torch.uint8)
        self._ws_mel_old = None


def test_same_bits_catches_each_kind_of_stale_read_with_the_fill_meant_for_it():
    """same_bits against passes written here, on the host, that let their workspace into the result the ways a kernel does:
    a stale word times zero (caught by 0xFF: 0 * NaN; not by 0x7B: 0 * 1.3e36 = 0), a stale word through fmax / fmin, which launder
    NaN (caught by 0x7B alone), a stale int32 used as a count, a result that differs from run to run, and a NaN in the output."""
    ctx = _FakeCtx(64)
    x = torch.arange(64, dtype=torch.float32)
    f32 = lambda t: t.view(torch.float32)
    assert torch.equal(P.same_bits(lambda: x * 2, ctx, finite=True)["out"], x * 2)          # a clean pass passes, and returns the baseline
    assert bool((ctx._ws == 0x7B).all()) and bool((ctx._ws_mel == 0x7B).all())              # ... and the last fill reached both workspaces
    with pytest.raises(AssertionError, match="0xff"):
        P.same_bits(lambda: x + 0.0 * f32(ctx._ws), ctx)
    assert torch.equal(P.same_bits(lambda: x + 0.0 * f32(ctx._ws), ctx, fills=(0x00, 0x7B))["out"], x)
    clamp = lambda: x + torch.fmin(torch.fmax(f32(ctx._ws_mel), torch.zeros(())), torch.ones(()))
    assert torch.equal(P.same_bits(clamp, ctx, fills=(0x00, 0xFF))["out"], x)               # fmax(NaN, 0) = 0: 0xFF sees nothing
    with pytest.raises(AssertionError, match="0x7b"):
        P.same_bits(clamp, ctx)
    with pytest.raises(AssertionError, match="0xff"):
        P.same_bits(lambda: {"n": ctx._ws.view(torch.int32)[:1] + 5, "x": x}, ctx, outputs=["n"])
    assert set(P.same_bits(lambda: {"n": ctx._ws.view(torch.int32)[:1] + 5, "x": x}, ctx, outputs=["x"])) == {"x"}
    calls = iter(range(100))
    with pytest.raises(AssertionError, match="not deterministic"):
        P.same_bits(lambda: x + next(calls), ctx)
    with pytest.raises(AssertionError, match="NaN or inf"):
        P.same_bits(lambda: x / x, ctx, finite=True)                                        # 0 / 0 in element 0, whatever the fill
    assert torch.equal(P.bits(torch.tensor([1.0, float("nan")])), P.bits(torch.tensor([1.0, float("nan")])))   # the same NaN is the same bits


def _prof_calls(text):
    """The first argument behind `ctx` of every si_prof_begin CALL in a source text."""
    out = []
    for m in re.finditer(r"\bsi_prof_begin\(ctx,\s*", text):
        depth, i = 0, m.end()
        while i < len(text) and not (depth == 0 and text[i] == ","):
            if text[i] == '"':                               # a literal: skip to its closing quote
                i = text.index('"', i + 1)
            elif text[i] in "([":
                depth += 1
            elif text[i] in ")]":
                depth -= 1
            i += 1
        out.append(text[m.end():i])
    return out


def test_every_launcher_is_in_exactly_one_family_list():
    assert len(set(P.SCRATCH_FAMILIES)) == len(P.SCRATCH_FAMILIES) and len(set(P.NO_SCRATCH_FAMILIES)) == len(P.NO_SCRATCH_FAMILIES)
    assert not set(P.SCRATCH_FAMILIES) & set(P.NO_SCRATCH_FAMILIES)
    listed = set(P.SCRATCH_FAMILIES) | set(P.NO_SCRATCH_FAMILIES)
    assert set(P.PREFIX_FAMILIES) <= listed
    seen, calls, mentions = set(), 0, 0
    for path in sorted(glob.glob(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "*.hip"))):
        with open(path) as f:
            text = f.read()
        mentions += text.count("si_prof_begin(")
        for arg in _prof_calls(text):
            calls += 1
            names = re.findall(r'"([^"]*)"', arg)
            if not names:
                # the name is built at run time ("<prefix>_<math>_<tile>"): the launcher's file names the prefix
                stem = os.path.basename(path)[:-len(".hip")]
                prefix = [p for p in P.PREFIX_FAMILIES if stem == p or stem.startswith(p + "_")]
                assert len(prefix) == 1, f"{path}: si_prof_begin({arg.strip()}, ...) builds its name at run time and the file is in no prefix family"
                assert re.search(r'"%s_[^"]*%%' % prefix[0], text), f"{path}: no format that begins with {prefix[0]}_"
                names = prefix
            for n in names:
                assert (n in P.SCRATCH_FAMILIES) != (n in P.NO_SCRATCH_FAMILIES), f"{path}: family {n!r} is not in exactly one of the two lists"
                assert P.family_of(n) == n
                seen.add(n)
    assert calls >= 50 and calls == mentions - 1             # the parser saw every call (api.hip's definition is the one that is none)
    assert seen == listed, f"listed but launched nowhere: {sorted(listed - seen)}"


def test_family_of_maps_run_time_names_to_their_prefix():
    for name, fam in (("tapgemm_f16_256x64", "tapgemm"), ("lingemm_bf16_128x128", "lingemm"), ("gemmcu_bf16_256x256", "gemmcu"),
                      ("respair_f16_c128_acc", "respair"), ("posconv_bf16_c48", "posconv"), ("upsample_f16_c64", "upsample"),
                      ("reschain_f16_c32", "reschain_f16_c32"), ("layernorm", "layernorm")):
        assert P.family_of(name) == fam
    assert P.family_of("tapgemmx") is None and P.family_of("new_kernel") is None
