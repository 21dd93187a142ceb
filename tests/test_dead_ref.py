"""tests/dead_ref.py checks itself: the contract on values written out by hand, the builders' own assertions on every
shape the GPU tests use, and each seeded mistake changing the expected rows of at least one case.  No GPU."""
import numpy as np
import pytest

from tests import dead_ref as R
from tests import detect_ref as D

f32 = np.float32
nan, inf = f32(np.nan), f32(np.inf)


def test_held_by_hand():
    held = lambda x, tol=0.0: R.dead_mask(np.asarray(x), R.HELD, tol=tol).astype(int).tolist()
    assert held(f32([1, 1, 2, 3, 4, 4])) == [1, 1, 0, 0, 1, 1]                    # pairs at (0, 1) and at (n - 2, n - 1)
    assert held(f32([5])) == [0] and held(np.int16([0])) == [0]                   # n = 1 is never held
    assert held(f32([2, 2])) == [1, 1]
    t = f32(0.25)
    assert held(f32([0, t, 9, 0, np.nextafter(t, f32(1))]), float(t)) == [1, 1, 0, 0, 0]    # |diff| == tol, and the next float above it
    assert held(f32([1, 0.0, -0.0, 2])) == [0, 1, 1, 0]                           # 0.0 - (-0.0) = 0
    assert held(f32([nan, nan, 1, inf, inf, -inf, -inf, 2])) == [0] * 8           # NaN neighbours; inf - inf = NaN
    assert held(f32([inf, inf, 7]), float("inf")) == [0, 1, 1]                    # inf - inf stays false, 7 - inf = -inf is within inf
    assert held(np.int16([32767, -32768, 0]), 1.0) == [0, 0, 0]                   # 65535, not the int16 wrap to -1
    assert held(np.int16([32767, -32768, 0]), 65535.0) == [1, 1, 1]
    assert held(np.int16([32767, -32768, 0]), 65534.0) == [0, 1, 1]
    assert R.link_mask(f32([3, 3, 3]), 0.0).tolist() == [False, True, True, False]     # no link at i = 0 and none to x[n]
    assert R.link_mask(f32([3, 3, 3]), 0.0, before=f32(3), after=f32(3)).tolist() == [False, True, True, False]


def test_threshold_by_hand():
    x = f32([0.25, -0.8125, nan, inf, -inf, 0.0])
    assert R.peak_ref(x) == f32(0.8125) and R.peak_ref(np.int16([5, -32768, 32767])) == f32(32768)
    assert R.peak_ref(f32([nan, inf, -inf])) == 0 and R.peak_ref(f32([nan])) == 0
    assert R.threshold_ref(f32([nan, nan]), 0.5, 1.0) == f32(0.5)                 # all NaN: peak 0, T = thr
    assert R.threshold_ref(x, 0.125, 0.0) == f32(0.125)                           # rel = 0: no peak
    assert R.threshold_ref(x, 0.125, 0.5) == f32(0.40625) and R.threshold_ref(x, 0.5, 0.5) == f32(0.5)
    pk = f32(0.9)
    while f32(1e-3) * pk == f32(1e-3 * float(pk)):
        pk = np.nextafter(pk, f32(1))
    T = R.threshold_ref(f32([0.1, -pk]), 0.0, 1e-3)
    assert T.dtype == f32 and T.tobytes() == (f32(1e-3) * pk).tobytes() and T != f32(1e-3 * float(pk))   # one fp32 multiply, bit for bit
    two = np.stack([f32([0.5, 0.25]), f32([0.125, -2.0])], axis=1)               # channel 0: 0.5, 0.125; channel 1: 0.25, -2
    assert [R.peak_ref(two, c) for c in (0, 1, -1)] == [0.5, 2.0, 2.0]
    assert R.dead_mask(f32([0, -0.0, nan, 1e-40]), R.QUIET).tolist() == [True, True, False, False]


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_a_zero_run_of_two_or_more_lies_inside_a_held_run(dtype):
    """held_tol = 0: every threshold-0 quiet run of at least two samples is a run of equal samples, so it lies inside a held run."""
    for seed in range(6):
        n = 3 * R.CHUNK + 11
        rng = np.random.default_rng(seed)
        x = (rng.integers(-3, 4, n)).astype(dtype)
        x[D.random_mask(n, 0.05, seed)] = 0
        if dtype is np.float32:
            x[::7] *= f32(-1)                                                     # some of the zeros are -0.0
        quiet, held = R.dead_runs_ref(x, R.QUIET, min_len=2), R.dead_runs_ref(x, R.HELD)
        assert len(quiet) > 20
        hs, he = held[:, 0], held[:, 0] + held[:, 1]
        for a, l in quiet.tolist():
            k = np.searchsorted(hs, a, side="right") - 1
            assert k >= 0 and hs[k] <= a and a + l <= he[k], (seed, a, l)
        assert np.array_equal(R.dead_mask(x, R.ANY), R.dead_mask(x, R.QUIET) | R.dead_mask(x, R.HELD))


def test_the_value_cases_hold_what_they_say():
    names = [c.name for c in R.value_cases()]                                     # (each asserted its hand-written mask on the way)
    assert len(names) == len(set(names)) == 19


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_every_builder_realises_its_masks(dtype):
    """Every shape the GPU tests run: the builders assert the intended masks themselves; here, that the traps are in place and that
    the situations the names promise are there."""
    for n in R.SEAM_N:
        cases = R.seam_cases(n, dtype)
        assert len(cases) % 3 == 0 and all(c.x.size == n and c.x.dtype == dtype for c in cases)
        for c in cases:
            assert c.before.tobytes() == c.x[0].tobytes() and c.after.tobytes() == c.x[-1].tobytes()
        held = [c for c in cases if c.kind == R.HELD]
        if n >= 2:
            assert any(len(c.rows()) for c in held)
        if n >= 9:
            pairs = np.concatenate([c.rows() for c in held if c.name.startswith("pairs across")])
            assert {int(a) + 1 for a, l in pairs if l == 2} == set(range(8, n, 8))          # every multiple of 8 that fits is straddled
        if n > R.CHUNK:
            assert any(int(c.rows()[:, 1].max(initial=0)) >= n - R.CHUNK + 1 for c in held)  # whole chunks inside one run
            lens = {ml: sorted({int(l) for _, l in c.rows()}) for c in held if c.name.startswith("lengths") for ml in [c.min_len]}
            assert lens[1][:3] == [4, 5, 6] and lens[5][0] == 5 and all(l >= 7 for l in lens[7]), lens
    for c in R.peak_position_cases(dtype):
        assert R._mag(np.asarray(c.before)) > R.peak_ref(c.x) and R._mag(np.asarray(c.after)) > R.peak_ref(c.x)
    for ch in (2, 3, 8):
        cases = R.channel_cases(ch, dtype)
        assert len(cases) == 3 * (ch + 1) + 3 and all(c.x.shape[1] == ch for c in cases)
        x = cases[0].x
        flat = x.reshape(-1)
        with np.errstate(invalid="ignore"):
            same = np.flatnonzero((flat[1:] == flat[:-1]) & np.isfinite(flat[1:].astype(np.float64))) + 1
        assert np.any(same % ch != 0) and np.any(same % ch == 0)                  # equal adjacent elements: inside a time, across times
    big = R.long_case(dtype)
    assert -(-big.x.size // R.CHUNK) == R.TILE + 3 and big.x.size - 3 == int(np.argmax(R._mag(big.x)))


@pytest.mark.parametrize("bug", R.MISTAKES)
def test_seeded_mistake_changes_the_expected_rows(bug):
    """Each mistake, seeded into the reference, changes the rows of at least one case: the cases can tell it from the contract."""
    hits = [c.name for c in R.all_cpu_cases() if not np.array_equal(c.rows(bug), c.rows())]
    print(f"{bug}: {len(hits)} cases differ, first: {hits[:3]}")
    assert hits, bug
    assert all(np.array_equal(c.rows(None), c.rows()) for c in R.value_cases())
