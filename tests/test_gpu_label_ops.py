"""The label and metric kernels, one by one, against their float64 definitions (tests/label_ref.py): the k-means
arg-min on both kernels (`kmeans_mfma_kernel` with its `kmeans_cnorm_kernel`; `kmeans_assign_kernel`), the codebook's cosine arg-max,
splice, gather and loss terms with `sum_terms_kernel`, `code_splice_kernel`, `mel_metrics_kernel` and `sisdr_kernel`.

A wrong label is not a rounding error, so the inputs are built for the places where an arg-min goes wrong: near-tie rows whose float64
gap is a few times the a-priori fp32 bound, at every row position of a tile and with the two candidates in one column tile, in two, and
across the 128-centroid block border; exact ties between duplicate centroids; NaN, infinite and overflowing rows next to finite ones.
tests/test_label_ref.py shows on the CPU that every row is a clear win in float64 and that these inputs catch seeded mistakes.  Every
err / bound is noted in one RatioSummary per family and printed by the last test."""
import numpy as np
import pytest
import torch

from speech_inpainting_amd.arch import HubertArch, VocoderArch
from tests import label_ref as L
from tests.harness import RatioSummary, build_engine, scoped_env

pytestmark = pytest.mark.gpu

SUMMARY = {name: RatioSummary() for name in ("k-means", "codebook", "mel_metrics", "sisdr")}
KERNELS = {"mfma": {}, "scalar": {"SI_KMEANS_MFMA": "0"}}              # (at D % 32 != 0 both settings are the scalar kernel)


def _engine(K=100, D=80, cb=None):
    """The engine whose context the calls go through, kept under a key; the codebook cases bring their own grid-quantised codebook."""
    state = None if cb is None else (None, None, torch.from_numpy(cb))
    return build_engine(HubertArch.tiny(codebook_dim=D), VocoderArch.tiny(), K, state=state, key=f"test_gpu_label_ops:{K}x{D}:{cb is not None}")


def _ctx():
    return _engine().ctx


def _kmeans(x, cent, kernel):
    """x: a numpy array, or a device tensor (the sliced case)."""
    xd = x if torch.is_tensor(x) else torch.from_numpy(x).cuda()
    with scoped_env(KERNELS[kernel]):
        lab, dist = _ctx().kmeans_assign(xd, torch.from_numpy(cent).cuda(), with_distance=True)
    return lab.cpu().numpy(), dist.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ k-means
@pytest.mark.parametrize("shape", list(L.KMEANS_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_kmeans_labels_and_distances_at_near_ties(shape):
    """Every label is the float64 arg-min -- no row is left out: each one's float64 gap exceeds twice the bound, the near-tie rows' by
    4 to 10 times -- and every distance lies within E + g(D + 4) |x|^2 of the float64 squared distance, on both kernels."""
    case = L.kmeans_case(*shape)
    for kernel in KERNELS:
        near, rest = L.kmeans_check(case, *_kmeans(case["x"], case["cent"], kernel))
        print(f"   {shape} {kernel}: dist err / bound near-tie rows {near:.4f}, members {rest:.4f}")
        SUMMARY["k-means"].note(f"kmeans {kernel}", near, rest)


def test_kmeans_rows_that_start_one_row_into_a_tensor():
    """feats[1:] of a contiguous tensor at D = 96: still 16-byte aligned (the MFMA kernel), every tile's origin one row off."""
    case = L.kmeans_case(66, 96, 129)
    full = torch.cat([torch.full((1, 96), 1e6), torch.from_numpy(case["x"])]).cuda()
    view = full[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0 and view.data_ptr() == full.data_ptr() + 4 * 96
    for kernel in KERNELS:
        near, rest = L.kmeans_check(case, *_kmeans(view, case["cent"], kernel))
        SUMMARY["k-means"].note(f"kmeans {kernel}", near, rest)


@pytest.mark.parametrize("D", [64, 80])
def test_kmeans_exact_ties_go_to_the_lowest_index(D):
    """Centroid 3 copied to index 4 (the same thread's next candidate in neither kernel, its neighbour in both), 11, 35 (another
    column tile), 131 (another 128-centroid block) and 256 (K = 257: a third block; the scalar kernel's thread 0 again): members of
    that cluster get label 3, with one copy at a time and with all of them."""
    for dup in [b for _, b in L.KMEANS_DUPS] + [None]:
        for K in sorted({257, 12 if dup is None else dup + 1}):
            case = L.kmeans_dup_case(D, K, dup)
            for kernel in KERNELS:
                lab, dist = _kmeans(case["x"], case["cent"], kernel)
                assert (lab == 3).all(), (D, K, dup, kernel, lab)
                near, rest = L.kmeans_check(case, lab, dist)
                SUMMARY["k-means"].note(f"kmeans {kernel}", near, rest)


@pytest.mark.parametrize("D,K", [(64, 129), (80, 129), (256, 257), (32, 2)])
def test_kmeans_non_finite_rows_get_a_label_in_range(D, K):
    """torch.argmin's rule: a row with one NaN and a row of NaNs get label 0; a row of +inf, of 1e30 and of 3e38 (the dot's products
    overflow) some label in [0, K); the finite rows of the same launch -- the near-tie rows of the same 32-row tile among them -- keep
    their float64 labels and distances.  No label of these launches is handed to another kernel."""
    case = L.kmeans_nonfinite_case(D, K)
    for kernel in KERNELS:
        lab, dist = _kmeans(case["x"], case["cent"], kernel)
        print(f"   D={D} K={K} {kernel}: labels of the non-finite rows {dict(zip(L.NONFINITE_ROWS.values(), lab[list(L.NONFINITE_ROWS)].tolist()))}")
        near, rest = L.kmeans_nonfinite_check(case, lab, dist)
        SUMMARY["k-means"].note(f"kmeans {kernel}", near, rest)


@pytest.mark.parametrize("D", [64, 80])
def test_kmeans_a_nan_centroid_wins_every_row_at_its_lowest_index(D):
    for K, bad in ((257, (37, 130, 256)), (3, (1, 2)), (130, (129,))):
        case = L.kmeans_case(40, D, K)
        for k in bad:
            case["cent"][k, D // 2] = np.nan
        assert L.argmin_rule(L.kmeans_scores(case["x"], case["cent"])[0]).tolist() == [bad[0]] * 40
        for kernel in KERNELS:
            lab, _ = _kmeans(case["x"], case["cent"], kernel)
            assert (lab == bad[0]).all(), (D, K, kernel, lab)


# ------------------------------------------------------------------------------------------------------------ codebook
def _two_clips(case):
    """The case's rows as clip 0 and, in reverse order, as clip 1: a kernel that read the wrong clip would answer in the wrong order."""
    both = {k: np.concatenate([case[k], case[k][::-1]]) for k in ("v", "kind", "want", "target")}
    return dict(case, **both), len(case["v"])


@pytest.mark.parametrize("K,D", L.CODEBOOK_SHAPES)
def test_codebook_metrics_frame_by_frame(K, D):
    """si_codebook_metrics (it writes no mel: any D <= 128) on a grid-quantised codebook: pred is the float64 cosine arg-max on every
    row (each a clear win by more than twice the bound; the near-tie rows by 8 times the bound; zero and NaN rows label 0; copies of
    centroid 5 label 5), terms and cos_pt within g(20) A."""
    case, F = _two_clips(L.codebook_case(K, D))
    eng = _engine(K, D, case["cb"])
    feats = torch.from_numpy(case["v"]).reshape(2, F, D).cuda()
    target = torch.from_numpy(case["target"]).reshape(2, F).cuda()
    loss, terms, pred, cpt = eng.ctx.codebook_metrics(feats, torch.zeros(2, dtype=torch.int32, device="cuda"), F, target)
    near, rest = L.codebook_check(case, pred.cpu().numpy().reshape(-1), terms.cpu().numpy().reshape(-1), cpt.cpu().numpy().reshape(-1))
    print(f"   K={K} D={D}: terms, cos_pt err / bound near-tie, dup and zero rows {near:.4f}, members {rest:.4f}")
    SUMMARY["codebook"].note("codebook_metrics", near, rest)
    assert torch.isnan(loss).all()                                      # the NaN row's term is in the sum


@pytest.mark.parametrize("K", L.SPLICE_KS)
def test_codebook_splice_in_both_forms(K):
    """si_codebook_splice and si_codebook_splice_spans at D = 80: the labels are the float64 arg-max, the spliced mel column is
    raw[label] bit for bit, and every other element of the mel keeps its bits."""
    D = 80
    case, F = _two_clips(L.codebook_case(K, D))
    eng = _engine(K, D, case["cb"])
    fr = L.codebook_frame(case["v"], case["tables"], case["target"])
    feats = torch.from_numpy(case["v"]).reshape(2, F, D).cuda()
    Tm = F + 2
    mel0 = torch.arange(2 * D * Tm, dtype=torch.float32).reshape(2, D, Tm) * 0.25 + 1000.0
    want = mel0.clone()
    want[:, :, :F] = torch.from_numpy(case["tables"]["raw"][fr["pred"]]).reshape(2, F, D).permute(0, 2, 1)
    bits = lambda t: t.cpu().contiguous().view(torch.int32)
    mel = mel0.cuda()
    lab = eng.ctx.codebook_splice(feats, torch.zeros(2, dtype=torch.int32, device="cuda"), F, mel)
    assert lab.cpu().numpy().reshape(-1).tolist() == fr["pred"].tolist()
    assert torch.equal(bits(mel), bits(want))
    order = np.random.default_rng(K).permutation(2 * F)                 # the frame table in a shuffled order
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32, device="cuda")
    mel = mel0.cuda()
    lab = eng.ctx.codebook_splice_spans(feats, i32(order // F), i32(order % F), mel)
    assert lab.cpu().numpy().tolist() == fr["pred"][order].tolist()
    assert torch.equal(bits(mel), bits(want))


def test_codebook_loss_sums_more_than_256_terms():
    """One launch of 3 x 100 frames: loss = the float64 sum of the returned fp32 terms rounded to fp32, to 1 ulp (sum_terms_kernel
    strides its 256 threads over 300 terms); one target out of range makes it NaN."""
    K, D = 100, 80
    case = L.codebook_case(K, D)
    eng = _engine(K, D, case["cb"])
    rows = case["v"][case["kind"] != "nan"]
    rng = np.random.default_rng(8)
    feats = torch.from_numpy(rows[rng.integers(0, len(rows), (3, 100))]).cuda().contiguous()
    target = torch.from_numpy(rng.integers(0, K, (3, 100))).cuda()
    pos = torch.zeros(3, dtype=torch.int32, device="cuda")
    loss, terms, _, _ = eng.ctx.codebook_metrics(feats, pos, 100, target)
    want = np.float32(terms.cpu().numpy().astype(np.float64).sum())
    assert terms.numel() == 300 and np.isfinite(want) and want > 10
    assert abs(float(loss[0]) - float(want)) <= float(np.spacing(want)), (float(loss[0]), float(want))
    target[2, 99] = K
    loss, terms, _, _ = eng.ctx.codebook_metrics(feats, pos, 100, target)
    assert torch.isnan(loss[0]) and torch.isnan(terms[2, 99]) and int(torch.isnan(terms).sum()) == 1


@pytest.mark.parametrize("K", L.SPLICE_KS)
def test_codebook_splice_of_given_labels_at_the_edges(K):
    """si_codebook_splice_labels: labels -1, 0, K - 1 and K at frame positions -1, 0, Tm - 1 and Tm, one clip per combination: the
    columns of the labels and positions in range are raw[label] bit for bit, nothing else changes."""
    D, Tm = 80, 5
    case = L.codebook_case(K, D)
    eng = _engine(K, D, case["cb"])
    combos = [(lab, pos) for lab in (-1, 0, K - 1, K) for pos in (-1, 0, Tm - 1, Tm)]
    mel0 = torch.arange(16 * D * Tm, dtype=torch.float32).reshape(16, D, Tm) * 0.5 - 7.0
    want = mel0.clone()
    for b, (lab, pos) in enumerate(combos):
        if 0 <= lab < K and 0 <= pos < Tm:
            want[b, :, pos] = torch.from_numpy(case["tables"]["raw"][lab])
    mel = mel0.cuda()
    eng.ctx.codebook_splice_labels(torch.tensor([[lab] for lab, _ in combos], dtype=torch.int64, device="cuda"),
                                   torch.tensor([pos for _, pos in combos], dtype=torch.int32, device="cuda"), mel)
    assert torch.equal(mel.cpu().view(torch.int32), want.view(torch.int32))
    assert int((want != mel0).any(1).sum()) == 4                        # labels 0 and K - 1 at positions 0 and Tm - 1


# ------------------------------------------------------------------------------------------------------------ the unit splice
@pytest.mark.parametrize("T", L.SPLICE_TS)
def test_code_splice_is_the_two_slice_assignments(T):
    rng = np.random.default_rng(T)
    clean, masked = rng.integers(0, 100, (3, T)), rng.integers(100, 200, (3, T))
    for ranges in L.code_splice_ranges(T):
        first, last = zip(*ranges)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
        got = _ctx().code_splice(torch.from_numpy(clean).cuda(), torch.from_numpy(masked).cuda(), i32(first), i32(last))
        assert np.array_equal(got.cpu().numpy(), L.code_splice(clean, masked, first, last)), (T, ranges)


# ------------------------------------------------------------------------------------------------------------ mel metrics, SI-SDR
@pytest.mark.parametrize("D,Ln", L.MEL_SHAPES)
def test_mel_metrics_of_three_different_clips(D, Ln):
    """Each clip's cosine, d2 and rmse against float64 within the derived bounds (label_ref.mel_metrics), with and without `center`;
    then the three edge pairs as one batch: identical inputs (cos 1, d2 = rmse = 0 exactly), an offset per frame (d2 = 0: the bin
    mean removes it), a frame equal to `center` (norm 0: cosine 0, the clip finite)."""
    case = L.mel_case(D, Ln)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for center in (case["center"], None):
        got = _ctx().mel_metrics(dev(case["a"]), dev(case["b"]), None if center is None else dev(center)).cpu().numpy().astype(np.float64)
        q = [np.abs(got[i] - val) / bound for i, (val, bound) in enumerate(L.per_clip(lambda a, b: L.mel_metrics(a, b, center), case["a"], case["b"]))]
        names = list(case["edges"])
        ea, eb = np.stack([case["edges"][k][0] for k in names]), np.stack([case["edges"][k][1] for k in names])
        edge = _ctx().mel_metrics(dev(ea), dev(eb), None if center is None else dev(center)).cpu().numpy().astype(np.float64)
        assert np.isfinite(edge).all() and np.isfinite(got).all()
        qe = []
        for i, (val, bound) in enumerate(L.per_clip(lambda a, b: L.mel_metrics(a, b, center), ea, eb)):
            err = np.abs(edge[i] - val)
            assert (err[bound == 0] == 0).all()                         # (a single frame of zero norm: the cosine is an exact 0)
            qe.append(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))
        assert edge[names.index("identical"), 1] == 0.0 and edge[names.index("identical"), 2] == 0.0
        print(f"   D={D} L={Ln} center={center is not None}: err / bound clips {np.max(q):.4f}, edge clips {np.max(qe):.4f}")
        SUMMARY["mel_metrics"].note("mel_metrics", float(np.max(qe)), float(np.max(q)))
        assert np.max(q) <= 1 and np.max(qe) <= 1, (q, qe)


@pytest.mark.parametrize("n", L.SISDR_NS)
def test_sisdr_of_three_different_clips(n):
    """Noise 0.5, 1e-2 and 1e-4 against the float64 definition within the derived bound; est = 0.7 ref exactly within the same bound
    (the expanded residual cancels there: the bound says by how much); a zero reference and a zero estimate give the definition's
    finite values."""
    ref, noise = L.sisdr_case(n)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for lv in L.SISDR_NOISE:
        est = (0.7 * ref.astype(np.float64) + lv * noise).astype(np.float32)
        got = _ctx().sisdr(dev(est), dev(ref)).cpu().numpy().astype(np.float64)
        want = L.per_clip(L.sisdr, est, ref)
        q = np.array([abs(got[i] - val) / bound for i, (val, bound) in enumerate(want)])
        print(f"   n={n} noise {lv}: {[f'{val:.4f} dB' for val, _ in want]}, err / bound {q.max():.4f}")
        SUMMARY["sisdr"].note("sisdr", float(q.max()) if lv == 0.0 else 0.0, float(q.max()) if lv != 0.0 else 0.0)
        assert np.isfinite(got).all() and (q <= 1).all(), (n, lv, got, want)
    est = np.stack([ref[0], np.zeros(n, np.float32), np.zeros(n, np.float32)])
    rf = np.stack([np.zeros(n, np.float32), ref[1], np.zeros(n, np.float32)])
    got = _ctx().sisdr(dev(est), dev(rf)).cpu().numpy().astype(np.float64)
    want = L.per_clip(L.sisdr, est, rf)
    assert np.isfinite(got).all() and got[1] == 0.0 and got[2] == 0.0 and want[1][0] == 0.0 and want[2][0] == 0.0
    q0 = abs(got[0] - want[0][0]) / want[0][1]
    SUMMARY["sisdr"].note("sisdr", float(q0), 0.0)
    assert q0 <= 1, (got, want)


def test_zz_summary_of_ratios():
    """(last in the file) the largest err / bound per family over every check above: seam and edge rows | the rest."""
    for family, summary in SUMMARY.items():
        summary.report("   SUMMARY " + family + " | {key}: max err/bound seam+edge rows {near:.4f}, the rest {rest:.4f} over {checks} checks")
