"""CPU: the reference of tests/invalid_ref.py against a table checked by hand, its case builders against their own claims, and every
seeded mistake against the cases -- each one must change some case's rows or some cleaned sample.  Exact: no tolerance anywhere."""
import numpy as np
import pytest

from tests import dead_ref as R
from tests import invalid_ref as V

f32 = np.float32


def test_the_hand_checked_table():
    rows = V.value_table()
    assert len(rows) == 58
    for name, dtype, v, c, want in rows:
        got = V.invalid_mask(v, c, None, dtype)
        assert got.shape == (1,) and bool(got[0]) is want, (name, got)
    # the table holds what the issue lists
    names = " | ".join(r[0] for r in rows)
    for w in V.NAN_BITS:
        assert f"{w:#010x}" in names
    for what in ("+inf", "-inf", "+FLT_MAX", "-FLT_MAX", "one step over c", "one step under c", "|v| == c", "-0.0", "subnormal",
                 "int16 -32768 at c = 32767", "int16 -32768 at c = 32768", "s24 -2^23 at c = 2^23 - 1", "s24 -2^23 at c = 2^23"):
        assert what in names, what
    # the four NaN patterns are NaNs with their payloads and signs kept
    nans = V.bits(V.NAN_BITS)
    assert np.all(np.isnan(nans)) and nans.view(np.uint32).tolist() == list(V.NAN_BITS)


def test_c_inf_is_exactly_not_finite_and_flt_max_is_the_same_set():
    rng = np.random.default_rng(0)
    words = np.concatenate([rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32),
                            np.uint32([0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0, 0x80000000, 1, 0x80000001]), np.uint32(V.NAN_BITS)])
    v = words.view(f32)
    assert np.array_equal(V.invalid_mask(v, V.INF), ~np.isfinite(v))
    assert np.array_equal(V.invalid_mask(v, V.FLT_MAX), ~np.isfinite(v))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(V.invalid_mask(v, 1.0), ~(np.abs(v) <= f32(1.0)))
    # PCM: nothing is invalid without a finite ceiling below full scale
    assert not V.invalid_mask(np.arange(-32768, 32768).astype(np.int16), V.INF).any()
    assert V.invalid_mask(np.arange(-32768, 32768).astype(np.int16), 32766.0).sum() == 3           # -32768, -32767, 32767
    assert V.invalid_mask(V.S24([V.LO24, -V.HI24, V.HI24, V.HI24 - 1]), float(V.HI24 - 1), None, V.S24).tolist() == [True, True, True, False]


def test_clean_stages_plus_zero_and_keeps_every_other_bit():
    x = np.concatenate([V.bits(V.NAN_BITS), f32([np.inf, -np.inf, 3e38, -0.0, 0.5, -1.0, 1e-45])])
    out = V.clean(x, 1.0)
    assert out.view(np.uint32).tolist() == [0] * 7 + [0x80000000] + x[8:].view(np.uint32).tolist()   # +0.0, and -0.0 kept as it is
    assert V.clean(x, V.INF).view(np.uint32).tolist() == [0] * 6 + x[6:].view(np.uint32).tolist()    # 3e38 is finite
    assert V.clean(np.int16([-32768, 32767, 32766, -5]), 32766.0).tolist() == [0, 0, 32766, -5]
    assert V.clean(np.int16([-32768, 32767]), V.INF).tolist() == [-32768, 32767]
    assert V.clean(V.S24([V.LO24, V.HI24 - 1]), float(V.HI24 - 1)).tolist() == [0, V.HI24 - 1]


def test_run_extraction_by_hand():
    nan = np.nan
    x = f32([nan, 0, 0, nan, nan, 0, np.inf, -np.inf, nan, 0])
    assert V.invalid_runs_ref(x).tolist() == [[0, 1], [3, 2], [6, 3]]
    assert V.invalid_runs_ref(x, min_len=2).tolist() == [[3, 2], [6, 3]] and V.invalid_runs_ref(x, min_len=4).shape == (0, 2)
    assert V.invalid_runs_ref(f32([0.5, 2.0, -2.0, 1.0]), 1.0).tolist() == [[1, 2]]
    two = np.stack([x, x[::-1]], axis=1)                                 # column 1: 0 nan -inf inf 0 nan nan 0 0 nan
    assert V.invalid_runs_ref(two, channel=0).tolist() == V.invalid_runs_ref(x).tolist()
    assert V.invalid_runs_ref(two, channel=1).tolist() == [[1, 3], [5, 2], [9, 1]]
    assert V.invalid_runs_ref(two, channel=-1).tolist() == [[3, 1], [6, 1]]


def test_the_builders_keep_their_claims():
    cases = V.all_cpu_cases()
    assert len(cases) > 150
    for case in cases:
        rows = case.rows()
        assert rows.dtype == np.int32 and (rows.shape[1:] == (2,))
        m = case.mask()
        assert m.shape == (case.x.shape[0],) and np.array_equal(rows, R.runs_of(m, case.min_len))
    for dtype in V.DTYPES:
        for n in V.SIZES:
            seams = [c for c in V.size_cases(n, dtype) if c.name.startswith("seams")]
            for c in seams:
                m = c.mask()
                assert m[0] and m[n - 1], c.name                         # samples 0 and n - 1
                for s in range(V.CHUNK, n, V.CHUNK):
                    assert m[s - 1] and m[s], c.name                     # a run across every chunk seam
        for ch in (2, 3, 8):
            assert len(V.channel_cases(ch, dtype)) == ch + 1
    assert V.long_case().x.size == 1026 * 2048 + 5


@pytest.mark.parametrize("bug", V.MISTAKES)
def test_every_seeded_mistake_shows(bug):
    """Each mistake changes the rows of at least one case, or -- the staging mistake -- a cleaned sample."""
    if bug == "minus_zero":
        x = f32([0.5, np.nan, 0.25])
        assert V.clean(x).view(np.uint32).tolist() != V.clean(x, bug=bug).view(np.uint32).tolist()
        assert V.clean(x).tolist()[1] == V.clean(x, bug=bug).tolist()[1] == 0.0      # equal as numbers: only the bits tell
        return
    hit = []
    for case in V.all_cpu_cases():
        a, b = case.rows(), case.rows(bug)
        if a.shape != b.shape or not np.array_equal(a, b):
            hit.append(case.name)
    assert hit, bug
    want = {"inf_valid": "float32", "nan_valid": "float32", "pcm_own_width": "int", "pcm_full_scale": "int", "adjacent_channel": "channels"}
    if bug in want:
        assert any(want[bug] in name for name in hit), (bug, hit[:4])
    if bug == "pcm_own_width":                                          # both widths wrap
        assert any("int16" in h for h in hit) and any("int32" in h for h in hit), hit[:6]
    if bug == "greater_equal":                                          # |v| == c is valid
        assert V.invalid_mask(f32([1.0]), 1.0).tolist() == [False] and V.invalid_mask(f32([1.0]), 1.0, bug).tolist() == [True]
