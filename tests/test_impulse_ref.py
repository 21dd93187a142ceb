"""The reference of si_impulse_runs (tests/impulse_ref.py) against hand-worked cases, against itself at 60 digits, against
the speech fixture, and against twelve seeded mistakes.  No GPU."""
import math

import numpy as np
import pytest

from tests import burst_ref as B
from tests import dead_ref as R
from tests import impulse_ref as I
from tests import level_ref as L

f64 = np.float64


@pytest.fixture(scope="module")
def evaluated():
    """Every CPU case once: (case, rows, T, float64 results, exact results)."""
    out = []
    for c in I.cpu_cases():
        rows, T, res = I.check(c, exact=True)                          # the three conditions are asserted in there
        ex = []
        I.impulse_mask(c.x, exact=True, results=ex, **{k: v for k, v in c.kw.items() if k != "min_len"})
        out.append((c, rows, T, res, ex))
    return out


def test_scalar_and_numpy_lag_sums_give_the_same_bits():
    rng = np.random.default_rng(0)
    for W, p in ((1024, 16), (777, 32), (9, 2), (3, 2), (40, 32)):
        w = rng.standard_normal(W)
        assert I._lags([float(v) for v in w], p, float) == I._lags_np(w, p)


def test_order_2_worked_by_hand():
    # x = 1, 2, 1, 0: one block, F = [0, 4).  r = (6 (1 + 1e-9), 4, 1) whatever the order of the eight partial sums (integers).
    x = np.array([1, 2, 1, 0], np.float32)
    r0, r1, r2 = 6.0 * (1.0 + 1e-9), 4.0, 1.0
    k1 = -r1 / r0
    E1 = r0 * (1.0 - k1 * k1)
    k2 = -(r2 + k1 * r1) / E1
    a1, a2 = k1 + k2 * k1, k2
    res = I.residual_ref(x, order=2)
    assert res.e[0] == 0.0 and res.e[1] == 0.0                        # t < p: no residual
    assert res.e[2] == (1.0 * 1.0 + a1 * 2.0) + a2 * 1.0 and res.e[3] == (1.0 * 0.0 + a1 * 1.0) + a2 * 2.0
    assert res.ratios == [E1 * (1.0 - k2 * k2) / r0]
    assert abs(a1 + 1.0) < 1e-6 and abs(a2 - 0.5) < 1e-6               # the normal equations of r = (6, 4, 1): a = (1, -1, 1/2)


def test_zero_file_single_click_and_shortest_files():
    assert I.impulse_runs_ref(np.zeros(700, np.float32), half=32)[0].shape == (0, 2)
    for n, t, pad, want in ((700, 300, 2, [[298, 5]]), (700, 699, 2, [[697, 3]]), (700, 17, 3, [[14, 7]]), (700, 16, 2, [[14, 5]]), (700, 15, 2, [])):
        x = np.zeros(n, np.int16)
        I.plant(x, t)
        assert I.impulse_runs_ref(x, half=32, pad=pad)[0].tolist() == want, (n, t)
    for p in (2, 16, 32):
        for n in (p, p + 1):
            x = I.signal(n, np.float32, 1)
            I.plant(x, n - 1)
            assert I.impulse_runs_ref(x, order=p, half=8, guard=0)[0].shape == (0, 2)
            assert np.all(I.residual_ref(x, order=p).e[:p] == 0.0)


def test_cnt_boundary():
    lo, hi = I.cnt_cases()
    assert I.check(lo)[0].tolist() == [] and I.check(hi)[0].tolist() == [[10, 1]]


def test_nan_inside_and_outside_a_fit_window():
    inside, outside = I.nan_cases()
    e_in, e_out = I.residual_ref(inside.x).e, I.residual_ref(outside.x).e
    assert np.isnan(e_in[512:1536]).all() and np.isfinite(e_in[:512]).all() and np.isfinite(e_in[1536:]).all()   # blocks 1 and 2 hold sample 1279
    assert np.isfinite(e_out[:1024]).all() and np.isnan(e_out[1024:]).all()         # sample 1280 is one past block 1's window
    clean = I.residual_ref(I.signal(2048, np.float32, 3)).e
    assert np.array_equal(e_out[:1024], clean[:1024])


def test_float64_decisions_equal_the_exact_ones_and_the_residual_error_is_measured(evaluated):
    worst = 0.0
    for c, rows, T, res, ex in evaluated:
        for a, b in zip(res, ex):
            assert np.array_equal(a.hot, b.hot) and np.array_equal(a.dead, b.dead), c.name
            for t, v in enumerate(b.e_exact):
                if v is not None and a.A[t] > 0:
                    worst = max(worst, float(abs(v - float(a.e[t]))) / a.A[t])
    print(f"worst |e64 - e_exact| / A = {worst:.3e} = 2^{math.log2(worst):.2f}; C_MEASURED = 2^{math.log2(I.C_MEASURED):.0f}, C_DEVICE = 2^{math.log2(I.C_DEVICE):.0f}")
    assert 0 < worst <= I.C_MEASURED and I.C_DEVICE == 16 * I.C_MEASURED <= 2.0 ** -24


def test_expected_rows_of_the_cases(evaluated):
    rows = {c.name.split("(")[0] + str(k): r.tolist() for k, (c, r, *_ ) in enumerate(evaluated)}
    assert rows["zeros0"] == [] and rows["zeros_click1"] == [[298, 5]] and rows["zeros_click2"] == [] and rows["zeros_click3"] == [[697, 3]]
    assert rows["voiced6"] == [[509, 6], [798, 6]] and rows["ar27"] == [[510, 6], [998, 6]] and rows["voiced8"] == [[512, 4]]
    assert rows["constant10"] == [] and rows["stereo11"] == [[698, 6]] and rows["T above the click14"] == []


def test_each_seeded_mistake_changes_some_case(evaluated):
    caught = {bug: [] for bug in I.MISTAKES}
    for c, rows, T, res, _ in evaluated:
        kw = {k: v for k, v in c.kw.items() if k != "min_len"}
        for bug in I.MISTAKES:
            rr = []
            r2, _T = I.impulse_runs_ref(c.x, bug=bug, after=c.after, results=rr, **kw)
            if not np.array_equal(r2, rows) or any(not np.array_equal(a.e, b.e, equal_nan=True) for a, b in zip(res, rr)):
                caught[bug].append(c.name)
    assert all(caught.values()), {k: v for k, v in caught.items() if not v}
    assert len(I.MISTAKES) >= 10
    named = {"fit_unclipped_n": "loud after n", "no_ridge": "constant", "cnt_untruncated": "zeros_click(n=10", "greater_equal": "zeros",
             "no_T": "T above the click", "adjacent_channel": "stereo", "running_sums": "loud_then_quiet"}
    for bug, name in named.items():
        assert any(n.startswith(name) for n in caught[bug]), (bug, caught[bug])


# ------------------------------------------------------------------------------------------------------------ the speech fixture
def test_clean_speech_gives_no_run_and_the_prototypes_scores():
    x = I.seg22()
    top = np.sort(I.score(x, 16, 254, 4))[-5:][::-1]
    assert [round(float(v), 2) for v in top] == [8.53, 7.55, 7.35, 7.32, 7.31]
    for xx in (x, I.seg22_scaled()):
        for ratio in (10.0, 12.0):
            for half in (254, 256):
                assert I.impulse_runs_ref(xx, 16, half, 4, 2, ratio)[0].shape == (0, 2)


TABLE = {2000: (20, 20, 0, 9), 4000: (28, 28, 0, 9), 8000: (31, 31, 0, 9), 16000: (36, 36, 0, 9)}


@pytest.mark.parametrize("amp", sorted(TABLE))
def test_planted_click_table(amp):
    """37 clicks of 1 to 3 samples, +-amp added, one every 997 samples, ratio 10, half 256, pad 2: (found, fully covered by a run, false hot
    samples, longest run) as THIS reference finds them with seg22_clicked's seeded lengths and signs (DESIGN.md 4.33 sets them beside the
    prototype's, whose lengths and signs were other draws)."""
    assert I.click_table(amp) == TABLE[amp]


def test_the_other_kinds_at_their_documented_settings_find_no_planted_click():
    x, clicks = I.seg22_clicked(16000)
    near = np.zeros(x.size, bool)
    for s, m in clicks:
        near[s:s + m] = True
    quiet = R.dead_mask(x, 1, 0.0)                                     # kind quiet at its default: exact zeros
    level = L.level_mask(x, 22, 33.0)                                  # kind level: win_ms = 2.0 at 22.05 kHz, a floor of 0.001 of full scale
    burst = B.burst_mask(x, 44, B.THR[np.int16])                       # kind burst: win_ms = 4.0, 1.15 of full scale
    for name, mask in (("quiet", quiet), ("level", level), ("burst", burst)):
        assert not (np.asarray(mask) & near).any(), name
