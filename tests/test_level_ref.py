"""The exact reference of si_level_runs (tests/level_ref.py), checked on the CPU: the contract by hand on tiny inputs,
the measurement that motivated the detector on the speech fixture, every case builder (each asserts that none of its samples depends
on the order of the additions), and the seeded mistakes -- each must change the expected rows of some case."""
import numpy as np
import pytest

from tests import dead_ref as R
from tests import level_ref as L

f32 = np.float32
_CASES = {}


def _cases():
    if not _CASES:
        _CASES["all"] = L.all_cpu_cases()
    return _CASES["all"]


def _mask(x, h, thr, **kw):
    return L.level_mask(np.asarray(x), h, thr, **kw).astype(int).tolist()


# ------------------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_the_contract_by_hand(dtype):
    a = lambda v: np.asarray(v, dtype=dtype)
    # truncated windows at both ends, one loud sample: its three windows are not low, the dilation leaves the sample itself
    assert _mask(a([0, 0, 0, 5, 0, 0, 0]), 1, 1.0) == [1, 1, 1, 0, 1, 1, 1]
    # an exact-zero dropout of 2 h + 1 samples in loud audio comes back as itself, one sample shorter is nothing
    x = np.full(20, 9, dtype=dtype)
    x[5:12] = 0
    assert L.level_runs_ref(x, 3, 1.0).tolist() == [[5, 7]]
    x[11] = 9
    assert L.level_runs_ref(x, 3, 1.0).tolist() == []
    # RMS, not peak: [1, 3, 1] has energy 11 <= 4 * 3, [3, 1, 3] has 19
    assert _mask(a([3, 1, 3, 1, 1, 3, 1, 3]), 1, 2.0, bug="no_dilation") == [0, 0, 1, 1, 1, 1, 0, 0]          # low(i) itself
    assert _mask(a([3, 1, 3, 1, 1, 3, 1, 3]), 1, 2.0) == [0, 1, 1, 1, 1, 1, 1, 0]                               # and its union
    assert _mask(a([3, 1, 3, 1, 1, 3, 1, 3]), 0, 2.0) == [0, 1, 0, 1, 1, 0, 1, 0]          # half 0: sample-wise
    # the file ends: cnt is the truncated count, [3, 1] has 10 > 4 * 2 while [1, 3, 1] passes
    assert _mask(a([3, 1, 1, 3, 1]), 1, 2.0, bug="no_dilation") == [0, 1, 1, 1, 0]
    # E == lim at every window, and one step under
    assert _mask(a([3] * 9), 2, 3.0) == [1] * 9 and _mask(a([3] * 9), 2, float(np.nextafter(f32(3), f32(0)))) == [0] * 9
    # min_len and the rows
    assert L.level_runs_ref(a([0, 0, 0, 5, 0, 0, 0, 0]), 1, 1.0, min_len=4).tolist() == [[4, 4]]
    # T = max(thr, fl32(rel * peak)): dead_ref's
    x = a([1000, 3, -3, 3, 1000, 4, 4, 4, 1000]) if dtype is np.int16 else a([0.5, 3e-3, -3e-3, 3e-3, 0.5, 4e-3, 4e-3, 4e-3, 0.5])
    rel = 3.5 / 1000 if dtype is np.int16 else 7e-3
    assert L.level_runs_ref(x, 1, 0.0, rel).tolist() == [[1, 3]] and L.level_runs_ref(x, 1, 0.0, 0.0).tolist() == []
    assert L.Case("T", x, 1, 0.0, rel).threshold() == R.threshold_ref(x, 0.0, rel)


def test_nan_inf_and_huge_samples():
    nan, inf = np.nan, np.inf
    assert _mask(f32([0, 0, nan, 0, 0, 0]), 1, 1.0) == [1, 1, 0, 1, 1, 1]                  # bad, not zero, and not poison
    assert _mask(f32([0, 0, inf, 0, 0, -inf]), 1, 1.0) == [1, 1, 0, 0, 0, 0]
    assert _mask(f32([1, 1, 3e38, 0, 0, 0, 0, 1, 1]), 1, 0.5) == [0, 0, 0, 1, 1, 1, 1, 0, 0]   # the run starts at p + 1
    assert _mask(f32([1, 1, 3e38, 0, 0, 0, 0, 1, 1]), 1, 0.5, bug="prefix_diff") == [0, 0, 0, 1, 1, 1, 1, 1, 1]
    assert _mask(np.int16([-32768] * 5), 1, 32768.0) == [1] * 5 and _mask(np.int16([-32768] * 5), 1, 32767.0) == [0] * 5
    assert _mask(np.int16([-32768] * 5), 1, 32767.0, bug="int32_squares") == [1, 1, 1, 1, 1]    # 3 * 2^30 wraps below zero


def test_interleaved_by_hand():
    x = np.int16([[0, 9], [0, 9], [0, 0], [9, 0], [9, 0], [9, 0]])
    assert _mask(x, 1, 1.0, channel=0) == [1, 1, 1, 0, 0, 0] and _mask(x, 1, 1.0, channel=1) == [0, 0, 1, 1, 1, 1]
    assert _mask(x, 1, 1.0, channel=-1) == [0, 0, 1, 0, 0, 0]
    assert _mask(x, 1, 1.0, channel=0, bug="adjacent_channel") != _mask(x, 1, 1.0, channel=0)
    one = x[:, :1]
    assert _mask(one, 1, 1.0, channel=0) == _mask(one, 1, 1.0, channel=-1) == _mask(one[:, 0], 1, 1.0)
    # joint: one T from the peak over all elements; a channel alone: its own
    y = np.int16([[1000, 10], [2, 10], [2, 2], [2, 2], [2, 2], [1000, 10]])
    assert L.Case("c1", y, 0, 0.0, 0.25, 1, 1).threshold() == f32(2.5) and L.Case("j", y, 0, 0.0, 0.25, 1, -1).threshold() == f32(250)


def test_the_measurement_on_the_speech_fixture():
    """The nine settings of the measurement: the sample-wise detector at T = 12 .. 84 and the windowed level at T = 16 and 20, runs of at
    least 110 samples, on seg22 with two 200 ms stretches of rint(N(0, 12))."""
    x = L.seg22_damaged()
    planted = [[8000, 4410], [24000, 4410]]
    rows = {T: R.dead_runs_ref(x, R.QUIET, float(T), 0.0, 0.0, 110).tolist() for T in (12, 24, 36, 48, 60, 72, 84)}
    inside = lambda r: [v for v in r if v[0] >= 1000]                  # the file's quiet lead-in apart
    assert rows[12] == []
    assert len(rows[24]) == 5 and max(l for _, l in rows[24]) < 300                         # five slivers
    assert len(rows[36]) == 19                                                              # 19 fragments
    assert inside(rows[48]) == [[8000, 4410], [24000, 247], [24248, 4162]]                  # the second dropout split in two
    for T in (60, 72, 84):
        assert inside(rows[T]) == planted and len(rows[T]) == 3, T
    for T in (16, 20):                                                                      # 11 dB below the first sample-wise threshold that works
        got = L.level_runs_ref(x, 22, float(T), 0.0, 110).tolist()
        assert inside(got) == planted and all(s + l < 1000 for s, l in got[:-2]), (T, got)
        assert np.array_equal(np.asarray(got), L.level_runs_ref(x.astype(f32), 22, float(T), 0.0, 110))     # the fp32 path: Python integers


# ------------------------------------------------------------------------------------------------------------ the cases
def test_every_case_is_decided_and_finds_something():
    cases = _cases()
    assert len(cases) > 400 and sum(len(c.rows()) > 0 for c in cases) > len(cases) // 3
    flat, start = cases[0].memory()
    assert np.array_equal(flat[start:start + cases[0].x.size], cases[0].x.reshape(-1))
    c = L.long_case()
    assert len(c.rows()) == 2


def test_an_undecided_sample_is_reported():
    """E = 4 + 1 + 2^-60 against lim = 5: the exact sum is above it, a float64 sum is 5.0 in every order."""
    c = L.Case("undecided", f32([2, 1, 0, 0, 2.0 ** -30]), 2, 1.0)
    assert c.undecided() == [2] and c.mask("no_dilation").astype(int).tolist() == [0, 0, 0, 1, 1]
    with pytest.raises(AssertionError):
        L.decided(c)
    assert L.Case("a tie that is a float64", f32([2, 1, 0, 0, 0]), 2, 1.0).undecided() == []


def test_half_zero_is_the_sample_wise_detector():
    for dtype in (np.float32, np.int16):
        assert len(L.half0_cases(dtype)) >= 8                          # the builder asserts the rows against dead_ref's


@pytest.mark.parametrize("bug", L.MISTAKES)
def test_a_seeded_mistake_changes_some_rows(bug):
    hits = [c.name for c in _cases() if not np.array_equal(c.rows(), c.rows(bug))]
    assert hits, bug
    if bug == "prefix_diff":
        assert any(name.startswith("a huge sample followed by zeros") for name in hits)
    if bug in ("past_n", "before_0"):
        assert any("file ends" in name for name in hits), hits[:5]
    if bug == "adjacent_channel":
        assert all("channels" in name for name in hits)
