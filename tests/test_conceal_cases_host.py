"""tests/conceal_cases.py held to its own claims, without a GPU: the covering set covers every pair of levels the engine's
refusals allow -- the allowed pairs recomputed here by brute force over the whole product --, holds no refused combination and at most 64
cases; every case's file is decided by its references and non-vacuous by them alone; every mended row meets the conditions under which
tests/test_gpu_mend.py states its bounds; and one forbidden call per constraint is refused by the engine's own code on a stand-in that
has no device, with the text the constraint restates."""
import itertools
import re

import numpy as np
import pytest
import torch

from speech_inpainting_amd import gaps as G
from speech_inpainting_amd.engine import InpaintingEngine
from tests import conceal_cases as CC
from tests import mend_ref as M
from tests.test_gpu_mend import _hold_condition

IDS, CASES = CC.covering_set()


def _per(case, value):
    """A per-channel value as a list of lists either way."""
    return value if CC.detect_of(case) == "each" else [value]


def test_the_covering_set_covers_every_allowed_pair():
    product = CC.product()
    assert len(product) == int(np.prod([len(levels) for _, levels in CC.FACTORS]))
    allowed, every = set(), set()
    for c in product:
        every.update(CC.pairs_of(c))
        if CC.refused(c) is None:
            allowed.update(CC.pairs_of(c))
    covered = set()
    for c in CASES:
        assert CC.refused(c) is None, c
        assert all(c[name] in levels for name, levels in CC.FACTORS)
        covered.update(CC.pairs_of(c))
    assert covered == allowed, sorted(allowed - covered)[:8]
    assert len(CASES) <= CC.MAX_CASES and len(set(IDS)) == len(IDS)
    # the pairs no served case holds are exactly those the table's constraints name
    gone = every - allowed
    assert gone == {p for p in every if _pair_refused(p)}, sorted(gone)[:8]
    print(f"   {len(CASES)} cases cover {len(covered)} of {len(allowed)} allowed pairs ({len(every)} pairs in all)")
    assert CC.covering_set() == CC.covering_set.__wrapped__(CC.SEED)   # deterministic


def _pair_refused(pair):
    """A pair no case can hold, written out from the constraints: 24-bit with feed="recording" or at 22 050 Hz, invalid with a relative
    threshold."""
    a, va, b, vb = pair
    d = {a: va, b: vb}
    return ((d.get("stype") == "s24" and d.get("feed") == "recording") or (d.get("stype") == "s24" and d.get("sr") == 22050)
            or (d.get("kind") == "invalid" and d.get("rel") == 1))


def test_the_refusal_table_names_every_constraint():
    assert set(CC.TABLE_CONSTRAINTS) <= set(CC.CONSTRAINTS) == set(CC.FORBIDDEN)
    hit = {CC.refused(c) for c in CC.product()}
    assert hit == set(CC.TABLE_CONSTRAINTS) | {None}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_case_is_decided_and_non_vacuous(case):
    e = CC.expected(case)                                              # an AssertionError here: no seed of 8 decides
    x = e["x"]
    ch = CC.CHANNELS[case["layout"]]
    assert x.dtype.type is CC.DTYPE[case["stype"]] and x.shape == ((x.shape[0],) if case["layout"] == "mono" else (x.shape[0], ch))
    assert x.shape[0] == CC.FRAMES * (case["sr"] // 50) + CC.TAIL
    gaps, skipped = _per(case, e["gaps"]), _per(case, e["skipped"])
    assert any(gaps), "no gap reaches the inpainter"
    assert not any(skipped), skipped                                   # no edge run, and no gap skipped as long: no case says so
    if CC.detect_of(case) == "each":
        assert len({tuple(g) for g in gaps}) >= 2, gaps
        if case["layout"] == "each3":
            assert gaps[1] == [] and e["rows"][1] == []
    if case["mend"] == "on":
        for mended, g in zip(_per(case, e["mended"]), gaps):
            if not mended and not g:
                continue                                               # the clean channel
            status = [st for _, _, st in mended]
            assert M.AR in status, status
        left = sum(len(g) for g in gaps)
        assert left >= 1
        assert e["mend"] and all(r.status.size == len(rows) for _, rows, r in e["mend"])
    else:
        assert "mended" not in e and e["mend"] == []
    if case["rel"]:
        for T in (e["threshold"] if CC.detect_of(case) == "each" else [e["threshold"]]):
            assert T != CC.threshold_of(case), T
    elif case["kind"] == "quiet":
        assert "threshold" not in e                                    # find_quiet_runs' launches: no T comes back
    # several contexts, so that batch = 2 is several passes: the planner's own grouping of these gaps
    n_rec, lim = CC.recording_frames(x.shape[0], case["sr"])
    assert n_rec == CC.FRAMES
    assert sum(len(G.plan_contexts(g, n_rec, CC.CLIP, CC.CTX, lim_frames=lim - (n_rec - CC.CLIP), fade_frames=1)) for g in gaps) >= (3 if case["batch"] == 2 else 2)


def test_the_mend_preconditions_hold_on_every_mended_row():
    """tests/test_gpu_mend.py's own conditions: E_p / r[0] > 1e-6 or r[0] == 0, and float64 within 2^-34 P of the 60-digit evaluation."""
    rows = 0
    for name, case in zip(IDS, CASES):
        if case["mend"] != "on":
            continue
        e = CC.expected(case)
        max_len, order, context = CC.mend_limits(case)
        flat = e["x"] if CC.CHANNELS[case["layout"]] >= 2 else e["x"].reshape(-1)
        for channel, runs, ref in e["mend"]:
            exact = M.mend(flat, runs, max_len, order, context, channel=channel, exact=True)
            _hold_condition(f"{name} channel {channel}", ref, exact)
            rows += sum(u is not None for u in ref.u)
    assert rows >= 3 * sum(c["mend"] == "on" for c in CASES)


def _stand_in():
    """An engine without a device: the engine's own methods on an object whose context is None, so that any launch is an AttributeError."""
    eng = object.__new__(InpaintingEngine)
    eng.device, eng.ctx = torch.device("cpu"), None
    eng._need = lambda **kw: None
    eng.recording_frames = lambda n22, clip_frames=200, n16=None: (n22 // 441, n22 // 441 - 1)
    return eng


@pytest.mark.parametrize("name", sorted(CC.FORBIDDEN))
def test_one_forbidden_call_per_constraint_is_refused_without_a_device(name):
    stype, sr, kw = CC.FORBIDDEN[name]
    with pytest.raises(ValueError, match=CC.CONSTRAINTS[name][1]):
        InpaintingEngine.conceal_file(_stand_in(), CC.forbidden_file(stype, sr), sr, **kw)


def test_the_refusals_of_the_table_agree_with_the_engine_on_the_whole_product():
    """refused() against conceal_file itself on the stand-in, for every combination of the factors the refusals read (kind, sample type,
    rate, feed, clips16, rel): refused with the named text, or served as far as the first launch."""
    eng = _stand_in()
    names = ("kind", "stype", "sr", "feed", "clips16", "rel")
    levels = dict(CC.FACTORS)
    for values in itertools.product(*(levels[k] for k in names)):
        case = dict(zip(names, values), layout="mono", mend="off", batch=32, input="host")
        why = CC.refused(case)
        try:
            InpaintingEngine.conceal_file(eng, CC.forbidden_file(case["stype"], case["sr"]), case["sr"], **CC.keywords(case))
            got = "served"
        except ValueError as err:
            got = str(err)
        except AttributeError as err:                                  # ctx is None: the call reached its first launch
            assert "NoneType" in str(err), err
            got = None
        assert got != "served"
        assert (got is None) if why is None else (got is not None and re.search(CC.CONSTRAINTS[why][1], got)), (case, why, got)
