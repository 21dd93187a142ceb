"""CPU: the float64 definitions behind the label and metric kernels (tests/label_ref.py) -- against the oracle's
functions on ordinary inputs, against three-element cases worked by hand, with seven seeded mistakes that the inputs and checks of
tests/test_gpu_label_ops.py each have to catch, and the condition those inputs rest on: every row is a clear win in float64, the
near-tie rows by 4 to 10 times twice the fp32 bound, with the winner as constructed and no row left out."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import label_ref as L


# ------------------------------------------------------------------------------------------------------------ against the oracle
def test_the_rules_are_torch_argmin_and_argmax():
    nan, inf = float("nan"), float("inf")
    rows = [[3.0, 1.0, 1.0, 2.0], [1.0, nan, 0.0, nan], [nan, nan, nan, nan], [inf, inf, inf, inf], [-inf, 0.0, -inf, 1.0],
            [0.0, -0.0, 0.0, -0.0], [2.0, 5.0, 5.0, nan]]
    v = np.array(rows)
    assert L.argmin_rule(v).tolist() == torch.argmin(torch.tensor(rows), dim=1).tolist() == [1, 1, 0, 0, 0, 0, 3]
    assert L.argmax_rule(v).tolist() == torch.argmax(torch.tensor(rows), dim=1).tolist() == [0, 1, 0, 0, 3, 0, 3]
    assert L.argmin_rule(v, "last_index_wins").tolist()[0] == 2 and L.argmin_rule(v, "nan_out_of_range").tolist()[1:4] == [L.INT_MAX] * 3


def test_kmeans_against_the_oracle_and_by_hand():
    g = torch.Generator().manual_seed(1)
    cent = torch.randn(50, 24, generator=g)
    x = cent[torch.randint(0, 50, (200,), generator=g)] + 0.8 * torch.randn(200, 24, generator=g)
    lab, dist = L.kmeans_assign(x.numpy(), cent.numpy())
    assert lab.tolist() == R.kmeans_assign(x, cent).tolist()
    assert np.allclose(dist, torch.cdist(x.double(), cent.double()).pow(2).min(1).values.numpy(), rtol=1e-12)
    # by hand: x = (1, 2, 2); c0 = (1, 2, 3): |c|^2 - 2 x.c = 14 - 22 = -8; c1 = (0, 0, 0): 0; c2 = (1, 2, 2): 9 - 18 = -9; |x|^2 = 9
    s, xx, E = L.kmeans_scores(np.array([[1.0, 2.0, 2.0]]), np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [1.0, 2.0, 2.0]]))
    assert s.tolist() == [[-8.0, 0.0, -9.0]] and xx.tolist() == [9.0]
    assert np.allclose(E, L.g(7) * np.array([[14 + 2 * 11, 0.0, 9 + 2 * 9]]), rtol=1e-15, atol=0) and L.g(7) == 7 * 2.0 ** -24 / (1 - 7 * 2.0 ** -24)
    assert L.kmeans_assign(np.array([[1.0, 2.0, 2.0]]), np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [1.0, 2.0, 2.0]]))[1].tolist() == [0.0]


def test_codebook_against_the_oracle_and_by_hand():
    rng = np.random.default_rng(2)
    cb = L.grid_codebook(100, 80, rng)
    t = L.codebook_tables(cb)
    centre, cc = R.codebook_tables(torch.from_numpy(cb))
    assert np.allclose(t["centre"], centre.numpy(), atol=1e-6) and np.allclose(t["cc"], cc.numpy(), atol=1e-6)
    assert np.abs(t["raw"] - cb).max() <= 2.0 ** -22 and np.allclose(t["rnorm"], 1.0 / np.linalg.norm(t["cc"], axis=1), rtol=1e-6)
    tgt = rng.integers(0, 100, 60)
    v = (t["cc"][rng.integers(0, 100, 60)] + 0.3 * rng.standard_normal((60, 80))).astype(np.float32)
    fr = L.codebook_frame(v, t, tgt)
    vt = torch.from_numpy(v)[None]
    assert fr["pred"].tolist() == R.codebook_argmax(vt, torch.from_numpy(cb))[0].tolist()
    loss, pred, cpt = R.cos_sim_loss(vt, torch.from_numpy(tgt)[None], torch.from_numpy(cb))
    assert abs(fr["term"].sum() - float(loss)) <= 1e-4 and pred[0].tolist() == fr["pred"].tolist() and np.abs(fr["cos_pt"] - cpt.numpy()).max() <= 1e-5
    # by hand: centroids (4, 0, 0), (0, 2, 0), (-4, -2, 0): centre 0; v = (3, 4, 0): cosines 3/5, 4/5, -20 / (5 sqrt 20)
    hand = dict(cc=np.array([[4.0, 0.0, 0.0], [0.0, 2.0, 0.0], [-4.0, -2.0, 0.0]], dtype=np.float32))
    fr = L.codebook_frame(np.array([[3.0, 4.0, 0.0]], dtype=np.float32), hand, [0])
    assert np.allclose(fr["cos"], [[0.6, 0.8, -4 / np.sqrt(20)]], rtol=1e-15) and fr["pred"].tolist() == [1]
    assert np.allclose(fr["term"], [0.4]) and np.allclose(fr["cos_pt"], [0.0]) and np.allclose(fr["amax"], [L.g(6) * 4 / np.sqrt(20)], rtol=1e-12, atol=0)   # A of centroid 2: (12 + 8) / (5 sqrt 20)
    tb = L.codebook_tables(np.array([[1.0, 0.0, 2.0], [3.0, 0.0, 0.0], [-1.0, 3.0, 1.0]], dtype=np.float32))
    assert tb["centre"].tolist() == [1.0, 1.0, 1.0] and tb["cc"].tolist() == [[0.0, -1.0, 1.0], [2.0, -1.0, -1.0], [-2.0, 2.0, 0.0]]
    assert np.allclose(tb["rnorm"], [1 / np.sqrt(2), 1 / np.sqrt(6), 1 / np.sqrt(8)], rtol=1e-7)
    with pytest.raises(AssertionError):
        L.codebook_tables(np.array([[0.1, 0.0]], dtype=np.float32))                           # off the grid: the mirror would depend on the order


def test_mel_metrics_and_sisdr_against_the_oracle_and_by_hand():
    c = L.mel_case(80, 57)
    for i in range(3):
        a, b = torch.from_numpy(c["a"][i]), torch.from_numpy(c["b"][i])
        val, bound = L.mel_metrics(c["a"][i], c["b"][i], c["center"])
        want = [float(t) for t in R.mel_signal_metrics(a, b, torch.from_numpy(c["center"]))]
        assert np.abs(val - want).max() <= 1e-5 * max(1.0, np.abs(val).max()) and (bound > 0).all() and (bound < 1e-3).all()
    # by hand, D = 3, L = 1: a = (1, 2, 3), b = (3, 2, 1): cos = 10 / 14; bin means 2, 2: e = (-2, 0, 2), sqrt(8 / 3)
    val, _ = L.mel_metrics(np.array([[1.0], [2.0], [3.0]]), np.array([[3.0], [2.0], [1.0]]))
    assert np.allclose(val, [10 / 14, L.LOG_SCALE * np.sqrt(8 / 3), L.LOG_SCALE * np.sqrt(8 / 3)], rtol=1e-15)
    ref, noise = L.sisdr_case(4099)
    for lv in (0.5, 1e-2, 1e-4):
        est = (0.7 * ref.astype(np.float64) + lv * noise).astype(np.float32)
        for i in range(3):
            val, bound = L.sisdr(est[i], ref[i])
            assert abs(val - R.sisdr(est[i], ref[i])) <= 2e-3 and 0 < bound < 1e-3                # (the oracle sums in fp32)
    # by hand: ref = (1, 0, 0), est = (1, 1, 0), eps -> a = (eps + 1) / (1 + eps) = 1; e_true = ref, e_res = (0, 1, 0): 10 log10(1) = 0
    assert abs(L.sisdr(np.array([1.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]))[0]) <= 1e-15
    # the definition's finite values for a zero reference and a zero estimate
    z = np.zeros(3, np.float32)
    assert np.isclose(L.sisdr(np.array([1.0, 1.0, 0.0]), z)[0], 10 * np.log10(L.EPS32 / (L.EPS32 + 2))) and L.sisdr(z, np.array([1.0, 0.0, 0.0]))[0] == 0.0
    assert L.sisdr(z, z)[0] == 0.0 and L.EPS32 == np.finfo(np.float32).eps


def test_code_splice_against_the_oracle_and_by_hand():
    rng = np.random.default_rng(4)
    clean, masked = rng.integers(0, 100, (1, 50)), rng.integers(100, 200, (1, 50))
    for fs, ms in ((3200, 1600), (0, 640), (15000, 5000), (320 * 50, 10)):
        want = R.code_splice(torch.from_numpy(clean[0]), torch.from_numpy(masked[0]), fs, ms)
        assert L.code_splice(clean, masked, [fs // 320], [(fs + ms) // 320])[0].tolist() == want.tolist()
    assert L.code_splice([[1, 2, 3]], [[7, 8, 9]], [1], [2]).tolist() == [[1, 8, 3]]
    assert L.code_splice([[1, 2, 3]], [[7, 8, 9]], [2], [1]).tolist() == [[1, 2, 3]] and L.code_splice([[1, 2, 3]], [[7, 8, 9]], [-1], [9]).tolist() == [[7, 8, 9]]


# ------------------------------------------------------------------------------------------------------------ the condition
@pytest.mark.parametrize("shape", list(L.KMEANS_SHAPES) + [(31, 64, 128), (33, 1024, 100), (66, 96, 129)])
def test_every_kmeans_row_is_a_clear_win_and_the_near_ties_are_near(shape):
    """kmeans_check asserts the condition itself before it looks at a kernel's output: here the definition is the kernel."""
    c = L.kmeans_case(*shape)
    near, rest = L.kmeans_check(c, *L.kmeans_assign(c["x"], c["cent"]))
    s, _, E = L.kmeans_scores(c["x"], c["cent"])
    w, gap = L.winner_gap(s, c["cent"])
    ratio = gap / (2 * E.max(1))
    print(f"   {shape}: {int(c['near'].sum())} near-tie rows, gap / 2E {ratio[c['near']].min(initial=np.inf):.2f} .. {ratio[c['near']].max(initial=0):.2f}; "
          f"the other rows from {ratio[~c['near']].min(initial=np.inf):.3g}")
    assert (near, rest) == (0.0, 0.0) and (ratio > 1).all()
    R_, D, K = shape
    assert int(c["near"].sum()) == (0 if K == 1 else 32 if R_ > 32 else R_ - R_ // 4)
    if K > 1 and R_ >= 8:
        assert len(set(c["want"][c["near"]].tolist())) >= 2               # the lower and the higher index both win rows
    if K >= 129 and R_ >= 32:
        assert {127, 128} <= set(c["want"][c["near"]].tolist())           # across the 128-centroid block border, both ways


@pytest.mark.parametrize("shape", L.CODEBOOK_SHAPES)
def test_every_codebook_row_is_a_clear_win_and_the_near_ties_are_near(shape):
    K, D = shape
    c = L.codebook_case(K, D)
    fr = L.codebook_frame(c["v"], c["tables"], c["target"])
    assert L.codebook_check(c, fr["pred"], fr["term"], fr["cos_pt"]) == (0.0, 0.0)
    kinds = set(c["kind"].tolist())
    assert {"member", "zero", "nan"} <= kinds and (("near" in kinds) == (K > 1 and D > 1)) and (("dup" in kinds) == (K > 6))
    if K > 135 and D > 1:
        assert {7, 135, 9, 10, 20, 84} <= set(c["want"][c["kind"] == "near"].tolist())      # one thread, neighbouring lanes, the two waves


# ------------------------------------------------------------------------------------------------------------ seeded mistakes
def _caught(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _kmeans_mistake(m):
    found = []
    for shape in L.KMEANS_SHAPES:
        c = L.kmeans_case(*shape)
        if _caught(L.kmeans_check, c, *L.kmeans_assign(c["x"], c["cent"], m)):
            found.append(("kmeans", shape))
    for D in (64, 80):
        for _, dup in L.KMEANS_DUPS:
            c = L.kmeans_dup_case(D, 257, dup)
            if _caught(L.kmeans_check, c, *L.kmeans_assign(c["x"], c["cent"], m)):
                found.append(("kmeans dup", D, dup))
        c = L.kmeans_nonfinite_case(D, 129)
        if _caught(L.kmeans_nonfinite_check, c, *L.kmeans_assign(c["x"], c["cent"], m)):
            found.append(("kmeans non-finite", D))
    return found


def _codebook_mistake(m):
    found = []
    for K, D in L.CODEBOOK_SHAPES:
        c = L.codebook_case(K, D)
        fr = L.codebook_frame(c["v"], c["tables"], c["target"], m)
        if _caught(L.codebook_check, c, fr["pred"], fr["term"], fr["cos_pt"]):
            found.append(("codebook", K, D))
    return found


def _within(val, want, bound):
    return bool((np.abs(np.asarray(val) - want) <= bound).all())


def _mel_mistake(m):
    found = []
    for D, Ln in L.MEL_SHAPES:
        c = L.mel_case(D, Ln)
        got = L.per_clip(lambda a, b: L.mel_metrics(a, b, c["center"], m)[0], c["a"], c["b"], mistake=m)
        want = L.per_clip(lambda a, b: L.mel_metrics(a, b, c["center"]), c["a"], c["b"])
        if not all(_within(g_, w, bd) for g_, (w, bd) in zip(got, want)):
            found.append(("mel", D, Ln))
        for name, (a, b) in c["edges"].items():
            val = L.mel_metrics(a, b, c["center"], m)[0]
            w, bd = L.mel_metrics(a, b, c["center"])
            if not (np.isfinite(val).all() and _within(val, w, bd)):
                found.append(("mel " + name, D, Ln))
    return found


def _sisdr_mistake(m):
    found = []
    for n in L.SISDR_NS:
        ref, noise = L.sisdr_case(n)
        est = (0.7 * ref.astype(np.float64) + 1e-2 * noise).astype(np.float32)
        got = L.per_clip(lambda e, r: L.sisdr(e, r)[0], est, ref, mistake=m)
        want = L.per_clip(L.sisdr, est, ref)
        if not all(abs(g_ - w) <= bd for g_, (w, bd) in zip(got, want)):
            found.append(("sisdr", n))
    return found


def _splice_mistake(m):
    found = []
    for T in L.SPLICE_TS:
        rng = np.random.default_rng(T)
        clean, masked = rng.integers(0, 100, (3, T)), rng.integers(100, 200, (3, T))
        for k, ranges in enumerate(L.code_splice_ranges(T)):
            first, last = zip(*ranges)
            if not np.array_equal(L.code_splice(clean, masked, first, last, m), L.code_splice(clean, masked, first, last)):
                found.append(("code_splice", T, k))
    return found


FAMILIES = (_kmeans_mistake, _codebook_mistake, _mel_mistake, _sisdr_mistake, _splice_mistake)


def test_no_check_objects_to_the_definition():
    assert [f(None) for f in FAMILIES] == [[], [], [], [], []]


@pytest.mark.parametrize("mistake", L.MISTAKES)
def test_each_seeded_mistake_is_caught(mistake):
    found = [hit for f in FAMILIES for hit in f(mistake)]
    print(f"   {mistake}: caught by {len(found)} cases, e.g. {found[:4]}")
    has = lambda *head: any(hit[:len(head)] == head for hit in found)
    if mistake == "dropped_eighth":
        assert all(has("kmeans", shape) for shape in L.KMEANS_SHAPES)                       # the near-tie rows: at every shape
    if mistake == "last_index_wins":
        assert all(has("kmeans dup", D, dup) for D in (64, 80) for _, dup in L.KMEANS_DUPS)
        assert all(has("codebook", K, D) for K, D in L.CODEBOOK_SHAPES if K > 6 and D > 1)  # the duplicates of centroid 5, the zero row
    if mistake == "nan_out_of_range":
        assert has("kmeans non-finite", 64) and has("kmeans non-finite", 80) and all(has("codebook", K, D) for K, D in L.CODEBOOK_SHAPES)
    if mistake == "clamp_after_division":
        assert all(has("codebook", K, D) for K, D in L.CODEBOOK_SHAPES)                     # the zero row: 0 / 0
        assert all(has("mel zero_norm", D, Ln) for D, Ln in L.MEL_SHAPES)
    if mistake == "mean_over_frames":
        assert all(has("mel", D, Ln) for D, Ln in L.MEL_SHAPES if D > 1 and Ln > 1) and all(has("mel offset", 80, Ln) for Ln in (255, 256, 257, 513))
    if mistake == "clip_zero":
        assert all(has("mel", D, Ln) for D, Ln in L.MEL_SHAPES if Ln > 1) and all(has("sisdr", n) for n in L.SISDR_NS)
    if mistake == "splice_off_by_one":
        assert all(has("code_splice", T, 1) for T in L.SPLICE_TS) and all(has("code_splice", T, 0) for T in L.SPLICE_TS if T > 1)
    assert found
