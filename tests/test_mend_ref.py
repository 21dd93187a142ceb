"""tests/mend_ref.py against itself: a hand-checked table, the quality the method was chosen for, and the seeded
mistakes -- each of which must change a status or a sample of some case, or the reference could not tell it from the definition.  No GPU."""
import math

import numpy as np
import pytest

from tests import mend_ref as M

f32 = np.float32


def _hand_file():
    """x[t] = cos(pi t / 2) over 17 samples, the sample at t = 8 (true value 1) damaged: K = 8, p = 2, m = 1."""
    x = np.array([1, 0, -1, 0, 1, 0, -1, 0, 99, 0, -1, 0, 1, 0, -1, 0, 1], dtype=f32)
    return x, [(8, 1)]


# ------------------------------------------------------------------------------------------------------------ the hand-checked table
def test_one_sample_with_order_two_worked_by_hand():
    """Each side holds four +-1: r[0] = 8 (1 + 1e-9); neighbours always meet a zero: r[1] = 0; three products of -1 per side: r[2] = -6.
    Levinson: kappa_1 = 0, kappa_2 = 6 / r[0] = kappa, a = (1, 0, kappa), b = (1 + kappa^2, 0, kappa).  B = [b0], d = -(b2 w[6] + b2 w[10]) =
    2 kappa, u = 2 kappa / (1 + kappa^2) = 0.96 at kappa = 0.75."""
    x, runs = _hand_file()
    res = M.mend(x, runs, 1, 2, 8)
    kap = 6.0 / (8.0 * (1.0 + 1e-9))
    want = 2.0 * kap / (1.0 + kap * kap)
    assert res.status.tolist() == [M.AR] and abs(res.u[0][0] - want) < 1e-15 and abs(want - 0.96) < 1e-9
    assert res.y[8] == f32(want) and np.array_equal(np.delete(res.y, 8), np.delete(x, 8)) and x[8] == 99
    assert abs(res.ratio[0] - (1.0 - kap * kap)) < 1e-15 and res.peak[0] == 1.0
    exact = M.mend(x, runs, 1, 2, 8, exact=True)
    assert exact.status.tolist() == [M.AR] and abs(float(exact.u[0][0]) - want) < 1e-15


def test_an_all_zero_context_is_the_line():
    x = np.zeros(40, f32)
    x[16:19] = 7.0
    res = M.mend(x, [(16, 3)], 8, 2, 8)
    assert res.status.tolist() == [M.LINE] and res.ratio == [None] and np.all(res.y == 0.0)
    x[15], x[19] = 0.0, 0.0                                             # and the line itself, where the fit fails late: a pivot of 0
    assert M.line(1.0, 5.0, 3) == [2.0, 3.0, 4.0]


def test_status_boundaries_one_sample_on_either_side():
    K, n = 8, 64
    x = M.as_type(M.voiced(n, 3), f32)
    st = lambda runs, **kw: M.mend(x, runs, kw.pop("max_len", 4), 2, K, **kw).status.tolist()
    assert st([(8, 2)]) == [M.AR] and st([(7, 2)]) == [M.EDGE]                                     # s - K = 0 against -1
    assert st([(n - 10, 2)]) == [M.AR] and st([(n - 9, 2)]) == [M.EDGE]                            # e + K = n against n + 1
    assert st([(20, 4)]) == [M.AR] and st([(20, 5)]) == [M.LONG]                                   # m = max_len against one more
    assert st([(-1, 2)]) == [M.BADROW] and st([(20, 0)]) == [M.BADROW] and st([(n - 1, 2)]) == [M.BADROW]
    assert st([(n - 2, 2)]) == [M.EDGE] and st([(0, 70)], max_len=64) == [M.BADROW] and st([(0, 64)], max_len=4) == [M.LONG]
    assert st([(10, 2), (20, 2)]) == [M.AR, M.AR]                                                  # a neighbour at exactly K behind the end
    assert st([(10, 2), (19, 2)]) == [M.NEAR, M.NEAR]                                              # and at K - 1
    assert st([(10, 2), (19, 30), (57, 2)], max_len=4) == [M.NEAR, M.LONG, M.EDGE]                 # LONG and EDGE come first; a LONG row is a neighbour
    y = x.copy()
    y[12] = np.nan                                                      # a NaN at s - K against s - K - 1
    assert M.mend(y, [(20, 2)], 4, 2, K).status.tolist() == [M.NONFINITE] and M.mend(y, [(21, 2)], 4, 2, K).status.tolist() == [M.AR]
    y = x.copy()
    y[30] = np.inf                                                      # the last context sample, e + K - 1, against e + K
    assert M.mend(y, [(20, 3)], 4, 2, K).status.tolist() == [M.NONFINITE] and M.mend(y, [(20, 2)], 4, 2, K).status.tolist() == [M.AR]
    y = x.copy()
    y[20:22] = np.nan                                                   # the damaged samples themselves are not read
    assert M.mend(y, [(20, 2)], 4, 2, K).status.tolist() == [M.AR] and np.all(np.isfinite(M.mend(y, [(20, 2)], 4, 2, K).y))
    big = np.full(n, f32(3e38))                                         # a finite context whose line leaves fp32: nothing is stored
    big[:20] = f32(-3e38)
    big[20:24] = 0
    res = M.mend(np.zeros(n, f32) + big, [(20, 4)], 4, 2, K)
    assert res.status.tolist() in ([M.NONFINITE], [M.AR], [M.LINE])


def test_rint_ties_and_the_clamps():
    s = lambda u, t: int(M.store(u, t))
    assert [s(u, np.int16) for u in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999, 2.50001)] == [0, 2, 2, 0, -2, -2, 0, 3]
    assert [s(u, np.int16) for u in (32766.5, 32767.49, 32767.5, 40000.0, 1e300)] == [32766, 32767, 32767, 32767, 32767]
    assert [s(u, np.int16) for u in (-32767.5, -32768.5, -32769.0, -1e300)] == [-32768, -32768, -32768, -32768]
    assert [s(u, M.S24) for u in (8388606.5, 8388607.5, 8388608.0, 1e12)] == [8388606, 8388607, 8388607, 8388607]
    assert [s(u, M.S24) for u in (-8388607.5, -8388608.5, -8388609.0, -1e12)] == [-8388608, -8388608, -8388608, -8388608]
    assert M.store(0.1, f32) == f32(0.1) and M.store(1e39, f32) == f32(np.inf)
    assert s(2.5, np.int16) != int(M.store(2.5, np.int16, bug="trunc")) + 1 and int(M.store(2.7, np.int16, bug="trunc")) == 2


def test_statuses_of_the_exact_path_are_the_float64_path_s():
    x = M.as_type(M.ar2(200, 5), np.int16)
    runs = [(40, 3), (60, 1), (120, 9), (190, 2)]
    a, b = M.mend(x, runs, 8, 4, 16), M.mend(x, runs, 8, 4, 16, exact=True)
    assert a.status.tolist() == b.status.tolist() == [M.AR, M.AR, M.LONG, M.EDGE] and np.array_equal(a.y, b.y)
    for ua, ub, P in zip(a.u, b.u, a.peak):
        if ua is not None:
            assert max(abs(float(p) - float(q)) for p, q in zip(ua, ub)) < 2.0 ** -34 * P


# ------------------------------------------------------------------------------------------------------------ quality
@pytest.mark.parametrize("m", [1, 8, 32])
def test_three_sinusoids_are_interpolated_far_better_than_by_the_line(m):
    """DESIGN.md 4.31's table: K = 512, p = 32; LSAR's maximum error is under 1e-2 of the peak and at least 10 x under the line's."""
    K, p = 512, 32
    n = 2 * K + m + 6
    truth = M.three_sines(n)
    x = truth.astype(f32)
    s = K + 3
    hurt = x.copy()
    hurt[s:s + m] = np.nan
    res = M.mend(hurt, [(s, m)], 64, p, K)
    peak = np.max(np.abs(truth))
    err = np.max(np.abs(np.array(res.u[0]) - truth[s:s + m])) / peak
    ln = np.max(np.abs(np.array(M.line(float(x[s - 1]), float(x[s + m]), m)) - truth[s:s + m])) / peak
    print(f"m = {m}: LSAR {err:.3g}, line {ln:.3g} of the peak")
    assert res.status.tolist() == [M.AR] and err < 1e-2 and err * 10 <= ln


# ------------------------------------------------------------------------------------------------------------ seeded mistakes
def _bank():
    """(name, x, runs, max_len, order, context, channel) cases for the seeded mistakes."""
    v = M.voiced(120, 11)
    st2 = np.stack([M.as_type(M.voiced(90, 1), np.int16), M.as_type(M.ar2(90, 2), np.int16)], axis=1)
    flat = np.full(40, f32(0.25))
    flat[16:18] = 9.0
    zero = np.zeros(40, f32)
    zero[16:19] = (5.0, 7.0, 2.0)
    hand, hruns = _hand_file()
    return [("hand", hand, hruns, 1, 2, 8, None),
            ("voiced fp32", M.as_type(v, f32), [(50, 5)], 8, 4, 16, None),
            ("voiced int16", M.as_type(v, np.int16), [(40, 3), (70, 6)], 8, 6, 24, None),
            ("ar2 s24", M.as_type(M.ar2(120, 4), M.S24), [(55, 4)], 8, 4, 16, None),
            ("all equal", flat, [(16, 2)], 4, 2, 8, None),
            ("all zero", zero, [(16, 3)], 4, 2, 8, None),
            ("near at K", M.as_type(v, f32), [(30, 2), (48, 2)], 4, 4, 16, None),
            ("edge at 0", M.as_type(v, f32), [(16, 2)], 4, 4, 16, None),
            ("edge at n", M.as_type(v, f32), [(102, 2)], 4, 4, 16, None),
            ("stereo", st2, [(40, 3)], 8, 4, 16, 0)]


def _differs(a, b):
    if a.status.tolist() != b.status.tolist() or a.y.tobytes() != b.y.tobytes():
        return True
    return any((p is None) != (q is None) or (p is not None and [float(v) for v in p] != [float(v) for v in q]) for p, q in zip(a.u, b.u))


@pytest.mark.parametrize("bug", M.MISTAKES)
def test_every_seeded_mistake_changes_a_status_or_a_sample(bug):
    hits = [name for name, x, runs, ml, p, K, c in _bank() if _differs(M.mend(x, runs, ml, p, K, channel=c), M.mend(x, runs, ml, p, K, channel=c, bug=bug))]
    print(bug, "->", hits)
    assert hits, bug
    want = {"no_ridge": "all equal", "line_inside": "all zero", "near_strict": "near at K", "edge_strict": "edge at 0", "adjacent_channel": "stereo",
            "trunc": "voiced int16"}
    assert bug not in want or want[bug] in hits, (bug, hits)


def test_the_bank_without_a_mistake_fills_what_it_should():
    got = {name: M.mend(x, runs, ml, p, K, channel=c).status.tolist() for name, x, runs, ml, p, K, c in _bank()}
    assert got["all zero"] == [M.LINE] and got["near at K"] == [M.AR, M.AR] and got["edge at 0"] == [M.AR] and got["edge at n"] == [M.AR]
    assert all(s in (M.AR, M.LINE) for v in got.values() for s in v), got
    assert math.isfinite(sum(float(np.sum(M.mend(x, runs, ml, p, K, channel=c).y.astype(np.float64))) for _, x, runs, ml, p, K, c in _bank()))
