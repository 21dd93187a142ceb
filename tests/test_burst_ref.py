"""The exact reference of si_burst_runs (tests/burst_ref.py), checked on the CPU: the contract by hand on tiny inputs,
the measurement that motivated the detector on the speech fixture, every case builder (each asserts that none of its samples depends
on the order of the additions), and the seeded mistakes -- each must change the expected rows of some case."""
import numpy as np
import pytest

from tests import burst_ref as B
from tests import dead_ref as R
from tests import level_ref as L

f32 = np.float32
_CASES = {}
T16 = float(f32(1.15 * 32768))


def _cases():
    if not _CASES:
        _CASES["all"] = B.all_cpu_cases()
    return _CASES["all"]


def _mask(x, h, thr, **kw):
    return B.burst_mask(np.asarray(x), h, thr, **kw).astype(int).tolist()


# ------------------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize("dtype", B.DTYPES)
def test_the_contract_by_hand(dtype):
    a = lambda v: np.asarray(v, dtype=dtype)
    # half 0: hot(i) <=> |d(i)| >= T for 1 <= i <= n - 2; samples 0 and n - 1 have no d.  d = [., 5, -10, 5, 0, .]
    x = a([0, 0, 5, 0, 0, 0])
    assert _mask(x, 0, 5.0) == [0, 1, 1, 1, 0, 0] and _mask(x, 0, 6.0) == [0, 0, 1, 0, 0, 0] and _mask(x, 0, 10.0) == [0, 0, 1, 0, 0, 0]
    assert _mask(x, 0, float(np.nextafter(f32(10), f32(11)))) == [0] * 6
    assert _mask(a([9, 0, 0, 0, 0, 9]), 0, 9.0) == [0, 1, 0, 0, 1, 0]                     # the end samples are neighbours, never centres
    # n < 3: no centre, no run, whatever the threshold; n = 3 has one
    for n in (1, 2):
        for h in (0, 1, 5):
            assert _mask(a([7, -7][:n]), h, 0.0) == [0] * n
    assert _mask(a([7, -7, 7]), 0, 28.0) == [0, 1, 0] and _mask(a([7, -7, 7]), 1, 28.0) == [1, 1, 1] and _mask(a([7, -7, 7]), 1, 29.0) == [0, 0, 0]
    # the truncated first and last windows: W(0) = [1, 1] at h = 1, cnt 1 -- E = 100 >= 64 * 1; an untruncated count of 3 would refuse it
    x = a([0, 5, 0, 0, 0, 0, 0])                                                            # d = [., -10, 5, 0, 0, 0, .]
    assert _mask(x, 1, 8.0, bug="no_dilation") == [1, 0, 0, 0, 0, 0, 0]                    # W(1) = [1, 2]: 125 < 128
    assert _mask(x, 1, 8.0) == [1, 1, 0, 0, 0, 0, 0]
    assert _mask(x, 1, 8.0, bug="cnt_full", ) == [0] * 7
    assert _mask(x[::-1].copy(), 1, 8.0) == [0, 0, 0, 0, 0, 1, 1]
    # a window that starts at 0 would difference sample 0 against what lies in front of the base
    assert _mask(a([0, 0, 0, 0]), 1, 8.0, before=a([100]), bug="window_from_0") == [1, 1, 1, 0] and _mask(a([0, 0, 0, 0]), 1, 8.0, before=a([100])) == [0] * 4
    # RMS over the window and >=: E == lim
    x = a([3, -3] * 5)                                                                       # |d| = 12 at every centre
    assert _mask(x, 2, 12.0) == [1] * 10 and _mask(x, 2, 12.0, bug="greater") == [0] * 10
    assert _mask(x, 2, float(np.nextafter(f32(12), f32(13)))) == [0] * 10
    # the dilation: one hot window at h = 2 reaches over 5 samples
    x = a([0, 0, 0, 0, 0, 40, 0, 0, 0, 0, 0, 0])                                            # d = 40, -80, 40 at 4, 5, 6: E(5) = 9600
    assert _mask(x, 2, 43.0, bug="no_dilation") == [0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0]    # 5 * 43^2 = 9245 <= 9600 (4 .. 6); E(3) = 8000
    assert _mask(x, 2, 43.0) == [0, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    # min_len, rows, and T = max(thr, fl32(rel * peak)): dead_ref's
    assert B.burst_runs_ref(x, 2, 43.0, min_len=8).tolist() == [] and B.burst_runs_ref(x, 2, 43.0, min_len=7).tolist() == [[2, 7]]
    assert B.burst_runs_ref(x, 2, 0.0, 43.0 / 40).tolist() == [[2, 7]] and B.Case("T", x, 2, 0.0, 1.075).threshold() == R.threshold_ref(x, 0.0, 1.075)


def test_the_integer_ranges():
    x = np.int16([32767, -32768] * 4)
    assert _mask(x, 1, 131070.0) == [1] * 8 and _mask(x, 1, 131071.0) == [0] * 8           # |d| = 131 070: no wrap
    assert _mask(x, 1, 131070.0, bug="int16_wrap") == [0] * 8                              # wrapped, d = -2
    assert _mask(x, 1, 65536.0, bug="int32_squares") == [0] * 8                            # 131070^2 mod 2^32 = 4, as int32
    v = np.array([B.HI24, B.LO24] * 4, dtype=B.S24)                                         # |d| = 2^25 - 2
    assert _mask(v, 1, 33554428.0) == [1] * 8 and _mask(v, 1, 33554432.0) == [0] * 8
    # 24-bit thresholds count 24-bit steps: the int16 file times 256 at the threshold times 256 has the int16 file's rows
    c = B.size_cases(2049, 7, np.int16)[4]
    assert np.array_equal(B.burst_runs_ref(c.x.astype(B.S24) * 256, 7, c.thr * 256, min_len=c.min_len), c.rows()) and len(c.rows()) > 0


def test_nan_inf_and_the_three_neighbour_rule():
    nan, inf = np.nan, np.inf
    x = f32([0, 0, 8, 0, 0, 0, 0, 0])                                                        # d = 8, -16, 8 at 1, 2, 3
    assert _mask(x, 0, 8.0) == [0, 1, 1, 1, 0, 0, 0, 0]
    for v in (nan, inf, -inf):
        y = x.copy(); y[4] = v                                                              # bad at centres 3, 4, 5: the three-neighbour rule
        assert _mask(y, 0, 8.0) == [0, 1, 1, 0, 0, 0, 0, 0]
        assert _mask(y, 1, 1.0, bug="no_dilation") == [1, 1, 0, 0, 0, 0, 0, 0]              # W(2) = [1, 3] holds bad(3); W(1) = [1, 2] does not
        y = x.copy(); y[0] = v                                                              # sample 0 is centre 1's neighbour
        assert _mask(y, 0, 8.0) == [0, 0, 1, 1, 0, 0, 0, 0]
    y = x.copy(); y[4] = inf
    assert _mask(y, 0, 8.0, bug="bad_centre_only") == [0, 1, 1, 1, 0, 1, 0, 0]              # an unjudged inf neighbour is an infinite level
    y = x.copy(); y[4] = nan
    assert _mask(y, 0, 8.0, bug="bad_centre_only") == [0, 1, 1, 0, 0, 0, 0, 0]              # NaN compares false either way
    # D in float64, two roundings: 1 - 2 * 0.5 + 3 2^-24 = 3 2^-24; in fp32 1 + 3 2^-24 is 1 + 2^-22
    x = f32([1.0, 0.5, 3 * 2.0 ** -24])
    assert _mask(x, 0, 3.5 * 2.0 ** -24) == [0, 0, 0] and _mask(x, 0, 3.5 * 2.0 ** -24, bug="fp32_D") == [0, 1, 0]
    assert _mask(x, 0, 3 * 2.0 ** -24) == [0, 1, 0]
    assert _mask(f32([3e38, -3e38, 3e38]), 0, 3.0e38) == [0, 1, 0]                           # |D| = 1.2e39, finite in float64


def test_interleaved_by_hand():
    # channel 0 alternates, channel 1 is flat; the ELEMENTS of the file are 4, 0, -4, 0, ...: no second difference along the file's elements at stride 1 equals either
    x = np.int16([[4, 1], [-4, 1], [4, 1], [-4, 1], [4, 1]])
    assert _mask(x, 0, 16.0, channel=0) == [0, 1, 1, 1, 0] and _mask(x, 0, 1.0, channel=1) == [0] * 5 and _mask(x, 0, 1.0, channel=-1) == [0] * 5
    assert _mask(x, 0, 16.0, channel=0, bug="adjacent_channel") == [0] * 5
    y = np.int16([[4, -4], [-4, 4], [4, -4], [-4, 4]])
    assert _mask(y, 0, 16.0, channel=-1) == [0, 1, 1, 0]
    # joint: ONE threshold from the peak over all elements
    z = np.int16([[4, 100], [-4, 100], [4, 100], [-4, 100]])
    assert _mask(z, 0, 0.0, rel=1.0, channel=0) == [0, 1, 1, 0] and _mask(z, 0, 0.0, rel=0.16, channel=-1) == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ the measurement
SEG22_ROWS = [[7988, 4472], [23973, 2270]]                              # what the reference computes; the issue's prototype found the same


def test_the_speech_fixture():
    """tests/golden/lj001_resample.npz: seg22 at h = 44 (4 ms at 22.05 kHz), T = fl32(1.15 * 32768): the clean file and its copy scaled
    to full scale give no run; the two planted blocks come back as exactly two runs, each containing its block."""
    assert B.burst_runs_ref(B.seg22(), 44, T16).tolist() == []
    assert np.abs(B.seg22_scaled().astype(np.int32)).max() == 32767 and B.burst_runs_ref(B.seg22_scaled(), 44, T16).tolist() == []
    rows = B.burst_runs_ref(B.seg22_damaged(), 44, T16).tolist()
    assert rows == SEG22_ROWS, rows
    for (s, l), (a, k) in zip(rows, B.BLOCKS):
        assert s <= a and s + l >= a + k


def test_the_other_detectors_find_neither_block():
    """Quiet, held and level detection at their documented settings on the damaged fixture: no run touches either block."""
    x = B.seg22_damaged()
    min_len = 110                                                       # 5 ms
    touches = lambda rows: [r for r in rows.tolist() for a, k in B.BLOCKS if r[0] < a + k and r[0] + r[1] > a]
    assert touches(R.dead_runs_ref(x, R.QUIET, 0.0, 0.0, 0.0, min_len)) == []
    assert touches(R.dead_runs_ref(x, R.HELD, 0.0, 0.0, 0.0, min_len)) == []
    assert touches(R.dead_runs_ref(x, R.ANY, 0.0, 2.0 ** -9, 0.0, min_len)) == []
    assert touches(L.level_runs_ref(x, 22, 32.0, 0.0, min_len)) == []   # win_ms = 2.0, a noise floor of 0.001 of full scale


# ------------------------------------------------------------------------------------------------------------ the builders
def test_every_builder_holds_its_own_assertions():
    cases = _cases()
    assert len(cases) > 200 and sum(len(c.rows()) for c in cases) > 200
    assert {c.x.dtype.type for c in cases} == set(B.DTYPES)


def test_the_sweep_is_the_thinned_product():
    sw = B.sweep()
    for h in B.HALVES:
        assert {(2049, h), (4101, h)} <= set(sw)
    for h in (0, 1, 1024):
        for n in (1, 2, 3, 4, 2047, 2048, 2049, 2050, 4101, 6144) + tuple(2 * g + k for g in B.HALVES for k in (1, 2, 3)):
            assert (n, h) in sw, (n, h)
    assert len(sw) == len(set(sw))


def test_the_long_case():
    c = B.long_case()
    assert c.x.size == 1026 * 2048 + 5 and len(c.rows()) == 2


@pytest.mark.parametrize("bug", B.MISTAKES)
def test_every_seeded_mistake_changes_some_case(bug):
    changed = [c.name for c in _cases() if not np.array_equal(c.rows(bug), c.rows())]
    assert changed, bug
