"""tests/extent.py on the CPU: guarded_allocs bands and restores, a planted byte is found wherever it lies and named
by its region, and every region the three passes of csrc/api.hip carve has a literal name of its own."""
import os
import re

import pytest
import torch

from tests import extent as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fills_are_the_two_nonzero_poison_bytes():
    assert X.FILLS == (0xFF, 0x7B)


@pytest.mark.parametrize("fill", X.FILLS)
def test_guarded_allocs_bands_every_allocation_and_restores_torch_empty(fill):
    real = torch.empty
    with X.guarded_allocs(fill, band=1024, device_type="cpu") as rec:
        assert torch.empty is not real
        a = torch.empty(3, 5, dtype=torch.float32, device="cpu")
        b = torch.empty((7,), dtype=torch.int64, device="cpu")
        c = torch.empty(0, dtype=torch.uint8, device="cpu")
        other = torch.empty(4)                                  # no device named: not this manager's business
        assert a.shape == (3, 5) and a.dtype == torch.float32 and a.is_contiguous() and b.shape == (7,) and c.numel() == 0
        assert len(rec.allocs) == 3 and [r[1] for r in rec.allocs] == [60, 56, 0]
        raw = rec.allocs[0][0]
        assert raw.numel() == 1024 + 60 + 1024 and bool((raw == fill).all()) and a.data_ptr() == raw.data_ptr() + 1024
        assert a.data_ptr() % 512 == raw.data_ptr() % 512
        a.zero_(); b.fill_(-1); other.zero_()                   # the tensor's own bytes are the caller's
        rec.check()
    assert torch.empty is real
    with pytest.raises(KeyError):
        with X.guarded_allocs(fill, band=512, device_type="cpu"):
            raise KeyError("the body raises")
    assert torch.empty is real


@pytest.mark.parametrize("fill", X.FILLS)
def test_a_byte_planted_in_a_band_is_found_on_either_side(fill):
    stray = X.FILLS[0] if fill != X.FILLS[0] else X.FILLS[1]    # a byte equal to ONE fill is caught under the other
    for at, words in ((1024 - 1, "byte 1 in front"), (1024 + 24, "byte 0 behind"), (1024 + 24 + 1023, "byte 1023 behind")):
        with X.guarded_allocs(fill, band=1024, device_type="cpu") as rec:
            t = torch.empty(2, 3, dtype=torch.float32, device="cpu")
            t.fill_(1.0)
            rec.check()
            rec.allocs[0][0][at] = stray
            with pytest.raises(AssertionError, match=rf"torch.empty\(\(2, 3\), torch.float32\).*{words}.*{stray:#04x}"):
                rec.check()
            rec.allocs[0][0][at] = fill                         # a stray store of the fill's own value is what the other fill is for
            rec.check()


REGIONS = [("lengths", 512, 24), ("stats", 1024, 256), ("h", 1792, 1000)]   # zone 512; slack behind lengths (232) and h (24)


def _ws(fill, size=4096):
    ws = torch.full((size,), fill, dtype=torch.uint8)
    for _, off, n in REGIONS:
        ws[off:off + n] = 0x11                                  # a pass writes its regions
    return ws


@pytest.mark.parametrize("fill", X.FILLS)
def test_a_planted_byte_is_found_in_a_zone_in_the_slack_and_behind_the_last_region(fill):
    stray = X.FILLS[0] if fill != X.FILLS[0] else X.FILLS[1]
    X.check_workspace(_ws(fill), REGIONS, fill)
    X.check_workspace(_ws(fill), list(reversed(REGIONS)), fill)  # the order given does not matter
    X.check_workspace(_ws(fill, 1792 + 1000), REGIONS, fill)     # a workspace that ends with its last region
    cases = ((0, "in front of the first region"), (511, "in front of the first region"),
             (512 + 24, "0 bytes behind the requested 24 bytes of region 'lengths'"),          # the slack up to the next 256
             (900, "364 bytes behind the requested 24 bytes of region 'lengths'"),             # the zone behind it
             (1280, "0 bytes behind the requested 256 bytes of region 'stats'"),
             (1792 + 1000, "0 bytes behind the requested 1000 bytes of region 'h'"),
             (4095, "1303 bytes behind the requested 1000 bytes of region 'h'"))               # the rest up to the end
    for at, words in cases:
        ws = _ws(fill)
        ws[at] = stray
        with pytest.raises(AssertionError, match=rf"workspace byte {at} holds {stray:#04x}, not the fill {fill:#04x}: {re.escape(words)}"):
            X.check_workspace(ws, REGIONS, fill)
        with pytest.raises(AssertionError):
            X.check_workspace(ws, REGIONS, stray)                # ... and under the other fill everything else is wrong
        ws[at] = fill
        X.check_workspace(ws, REGIONS, fill)
    with pytest.raises(AssertionError, match="leaves the workspace"):
        X.check_workspace(_ws(fill, 2000), REGIONS, fill)


def test_unchanged_holds_inputs_to_their_bits():
    x, n = torch.arange(12, dtype=torch.float32).reshape(3, 4), torch.tensor([1, 2, 3], dtype=torch.int32)
    x[0, 0] = float("nan")                                      # the same NaN is the same bits
    snap = X.unchanged({"x": x, "n": n, "absent": None})
    snap.check()
    x[2, 1] = -x[2, 1]
    with pytest.raises(AssertionError, match=r"input 'x' of shape \(3, 4\) was written: 1 elements differ, the first at flat index 9"):
        snap.check()
    x[2, 1] = -x[2, 1]
    n[0] = 0
    with pytest.raises(AssertionError, match="input 'n'"):
        snap.check()
    X.unchanged([x, None, n]).check()


# ------------------------------------------------------------------------------------------------------------ region names
PASSES = {"encoder": "hubert_run", "vocoder": "hifigan_run", "mel": "mel_run"}


def _body(text, fn):
    """The body of the DEFINITION of the static function `fn` in a source text: from the `{` behind its signature to its match."""
    starts = [m.end() for m in re.finditer(r"\bstatic int %s\([^;{]*\)\s*\{" % fn, text)]
    assert len(starts) == 1, (fn, len(starts))
    depth, i = 1, starts[0]
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[starts[0]:i]


def _carve_calls(text):
    """The last argument of every W.floats( / W.bytes( CALL of a source text."""
    out = []
    for m in re.finditer(r"\bW\.(?:floats|bytes)\(", text):
        depth, i, last = 0, m.end(), m.end()
        while not (depth == 0 and text[i] == ")"):
            if text[i] == '"':
                i = text.index('"', i + 1)
            elif text[i] in "([":
                depth += 1
            elif text[i] in ")]":
                depth -= 1
            elif text[i] == "," and depth == 0:
                last = i + 1
            i += 1
        out.append(text[last:i].strip())
    return out


def test_every_carve_call_names_its_region_and_no_pass_has_two_of_a_name():
    with open(os.path.join(ROOT, "speech_inpainting_amd", "csrc", "api.hip")) as f:
        text = f.read()
    literal = re.compile(r'^"([a-z][a-z0-9_]{0,22})"$')
    every = _carve_calls(text)
    assert len(every) == text.count("W.floats(") + text.count("W.bytes(") >= 30
    for arg in every:
        assert literal.match(arg), f"a carve call whose last argument is {arg!r}, not a short literal name"
    table = _carve_calls(text[text.index("int vl_table("):text.index("struct EncDims")])   # the ragged passes' table: one call, shared
    assert table == ['"lengths"']
    seen = 0
    for which, fn in PASSES.items():
        body = _body(text, fn)
        names = [literal.match(a).group(1) for a in _carve_calls(body)]
        assert body.count("vl_table(ctx, W,") == 1, (which, "the pass's length table")
        names.append("lengths")
        assert len(names) == len(set(names)), (which, sorted(n for n in names if names.count(n) > 1))
        assert 4 <= len(names) <= 32, (which, len(names))
        assert re.search(r"Carver W = carver\(ctx, SI_WS_%s," % which.upper(), body), which
        seen += len(names) - 1
    assert seen + 1 == len(every)                               # the three passes and vl_table hold every carve call of the file
    assert 'SI_WS_MAX_REGIONS 32' in open(os.path.join(ROOT, "include", "si_hip.h")).read()
