"""Float64 definitions of the label and metric kernels -- the k-means arg-min, the codebook's cosine arg-max with its
loss terms, the unit splice, the mel metrics and SI-SDR -- each on the fp32 operands the kernel reads, with the a-priori fp32 error
bounds the GPU tests hold the kernels to, the constructions of the inputs those tests use (near-tie rows, duplicate centroids,
non-finite rows) and the checks themselves, so that tests/test_label_ref.py can show on the CPU that the checks catch seeded mistakes.

Plain numpy.  u = 2^-24 is the unit roundoff of fp32 and g(n) = n u / (1 - n u) bounds the relative error of n roundings in a row.
A `mistake` argument seeds one of MISTAKES into a definition; None is the definition."""
import numpy as np

U = 2.0 ** -24
INT_MAX = 0x7fffffff
LOG_SCALE = 20.0 / np.log(10.0)
MISTAKES = ("dropped_eighth", "last_index_wins", "nan_out_of_range", "clamp_after_division", "mean_over_frames", "clip_zero",
            "splice_off_by_one")


def g(n):
    return n * U / (1.0 - n * U)


def f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ the two rules
def _rule(v, sign, mistake=None):
    v = np.asarray(v, dtype=np.float64)
    nan = np.isnan(v)
    key = np.where(nan, -np.inf, sign * v)                             # smallest key wins; a NaN beats every number
    K = v.shape[-1]
    if mistake == "last_index_wins":                                   # `<=` where the rule says `<`
        out = K - 1 - key[..., ::-1].argmin(-1)
    else:
        out = key.argmin(-1)                                           # numpy: the first of several equals
    if mistake == "nan_out_of_range":                                  # no comparison with a NaN, or with +inf against +inf, is true
        dead = nan.any(-1) | (key == np.inf).all(-1)
        out = np.where(dead, INT_MAX, out)
    return out.astype(np.int64)


def argmin_rule(v, mistake=None):
    """torch.argmin over the last axis: a NaN beats every number; among equals, and among NaNs, the lowest index wins."""
    return _rule(v, 1.0, mistake)


def argmax_rule(v, mistake=None):
    """torch.argmax over the last axis: a NaN beats every number; among equals, and among NaNs, the lowest index wins."""
    return _rule(v, -1.0, mistake)


def winner_gap(scores, table, sign=1.0):
    """Per row: the rule's winner w and the distance of its score to the best score among the RIVALS, the columns whose row of
    `table` (K, D) is not a bit-for-bit copy of row w (copies tie exactly in the kernels too: the rule decides them).  inf without a
    rival or where the scores are not finite.  sign 1: arg-min, -1: arg-max."""
    s = sign * np.asarray(scores, dtype=np.float64)
    w = _rule(scores, sign)
    tb = np.ascontiguousarray(np.asarray(table, dtype=np.float32)).view(np.uint32)
    gap = np.full(s.shape[0], np.inf)
    for r in range(s.shape[0]):
        rival = (tb != tb[w[r]]).any(1)
        if rival.any() and np.isfinite(s[r]).all():
            gap[r] = s[r, rival].min() - s[r, w[r]]
    return w, gap


# ------------------------------------------------------------------------------------------------------------ k-means
def kmeans_scores(x, cent, mistake=None):
    """x (R, D), cent (K, D) fp32 -> float64 s[r, k] = |c_k|^2 - 2 x_r . c_k, |x_r|^2 (R), and the fp32 bound
    E[r, k] = g(D + 4) (sum c^2 + 2 sum |x c|) on a computed s: the scalar kernel runs one D-long fma chain for the dot and one for
    |c|^2 and rounds `cc - 2 dot` once (D + 1 roundings on every term); the MFMA kernel runs eight D/8-long chains per dot (four
    waves, two lane halves), joins them with three adds, takes |c_k|^2 from a D/256-long chain, six shuffle adds and three adds, and
    rounds the same difference (at most D/8 + 4 on a dot term, 11 on a |c|^2 term at D <= 256).  D + 4 covers both."""
    x, c = f64(x), f64(cent)
    D = x.shape[1]
    with np.errstate(all="ignore"):
        cc = (c * c).sum(1)
        keep = D - D // 8 if mistake == "dropped_eighth" else D        # the last lane-half's share of the reduction is lost
        dot = x[:, :keep] @ c[:, :keep].T
        s = cc[None, :] - 2.0 * dot
        xx = (x * x).sum(1)
        E = g(D + 4) * (cc[None, :] + 2.0 * (np.abs(x) @ np.abs(c).T))
    return s, xx, E


def kmeans_assign(x, cent, mistake=None):
    """-> (labels int64 (R), squared distance to the winner float64 (R)) by the definition (or with a seeded mistake)."""
    s, xx, _ = kmeans_scores(x, cent, mistake)
    lab = argmin_rule(s, mistake)
    with np.errstate(all="ignore"):
        dist = s[np.arange(len(lab)), np.minimum(lab, s.shape[1] - 1)] + xx
    return lab, dist


def _pairs(K, wanted):
    """Those of the wanted index pairs that exist among K centroids and share no index with an earlier one."""
    used, out = set(), []
    for a, b in wanted:
        if 0 <= a < K and 0 <= b < K and a != b and not {a, b} & used:
            out.append((a, b))
            used |= {a, b}
    return out


KMEANS_PAIRS = ((0, 1), (2, 40), (127, 128), (5, -1))      # same MFMA column tile | two column tiles | the 128-centroid border | to K - 1
KMEANS_DUPS = ((3, 4), (3, 11), (3, 35), (3, 131), (3, 256))


def kmeans_case(R, D, K, seed=0):
    """Centroids N(0, 1); rows = noisy members of random centroids, and near-tie rows: at most 32 of them, row r < 32 (every tile
    position when R > 32; three of four when R <= 32, so that members remain) is the midpoint of centroids a and b pushed toward the
    one meant to win until the float64 gap of the two scores is 8 (E_a + E_b) -- between 4 and 8 times twice the row's largest E.
    The b of a pair is a + 0.5 N(0, 1), so that no third centroid comes near the midpoint.  -> dict(x, cent fp32; near bool (R);
    want int64 (R): the constructed winner, -1 for members' rows whose winner the float64 arg-min decides)."""
    rng = np.random.default_rng(1000 * seed + 7 * R + 3 * D + K)
    cent = rng.standard_normal((K, D)).astype(np.float32)
    pairs = _pairs(K, [(a, b if b >= 0 else K + b) for a, b in KMEANS_PAIRS])
    for a, b in pairs:
        cent[b] = cent[a] + (0.5 * rng.standard_normal(D)).astype(np.float32)
    x = (cent[rng.integers(0, K, R)] + 0.7 * rng.standard_normal((R, D))).astype(np.float32)
    near, want = np.zeros(R, bool), np.full(R, -1, np.int64)
    c64 = f64(cent)
    for r in range(min(R, 32)):
        if not pairs or (R <= 32 and r % 4 == 3):
            continue
        a, b = pairs[r % len(pairs)]
        if (r // len(pairs)) % 2:
            a, b = b, a                                                # the higher index wins these
        mid, dv = 0.5 * (c64[a] + c64[b]), c64[a] - c64[b]
        row = mid
        for _ in range(3):                                             # E depends (weakly) on the row: a fixed point
            _, _, E = kmeans_scores(row[None].astype(np.float32), cent[[a, b]])
            row = mid + 8.0 * E.sum() / (2.0 * (dv @ dv)) * dv         # s_b - s_a = 2 t |a - b|^2 at mid + t (a - b)
        x[r], near[r], want[r] = row.astype(np.float32), True, a
    return dict(x=x, cent=cent, near=near, want=want)


def kmeans_check(case, labels, dist):
    """Hold a kernel's (labels, dist) to the float64 definition on a kmeans_case: every row must be clear (gap > 2 E, E the row's
    largest), near-tie rows between 4 and 10 times that, the constructed winners win, every label the float64 arg-min, every dist within
    E + g(D + 4) |x|^2 of the float64 squared distance.  -> max err / bound over (near-tie rows, the rest)."""
    x, cent = case["x"], case["cent"]
    s, xx, E = kmeans_scores(x, cent)
    w, gap = winner_gap(s, cent)
    Er = E.max(1)
    fin = case.get("finite", np.ones(len(w), bool))                    # (all rows, but for the non-finite rows of kmeans_nonfinite_case)
    assert (gap[fin] > 2 * Er[fin]).all(), ("rows that are no clear win", np.nonzero(fin & ~(gap > 2 * Er))[0])
    near = case["near"]
    ratio = gap[near] / (2 * Er[near])
    want = case["want"]
    assert ((ratio >= 4) & (ratio <= 10)).all() and (w[want >= 0] == want[want >= 0]).all(), (ratio, w[want >= 0])
    labels, dist = np.asarray(labels), np.asarray(dist, dtype=np.float64)
    bad = fin & (labels != w)
    assert labels.shape == w.shape and not bad.any(), ("labels", np.nonzero(bad)[0][:8], labels[bad][:8], w[bad][:8])
    R = np.arange(len(w))
    with np.errstate(all="ignore"):
        q = np.abs(dist - (s[R, w] + xx)) / (E[R, w] + g(x.shape[1] + 4) * xx)
    assert np.isfinite(q[fin]).all() and (q[fin] <= 1).all(), ("dist: err / bound", np.nonzero(fin & ~(q <= 1))[0][:8], q[fin].max())
    edge = case.get("edge", near)                                      # what the summary counts as seam and edge rows
    return float(q[fin & edge].max(initial=0.0)), float(q[fin & ~edge].max(initial=0.0))


# ------------------------------------------------------------------------------------------------------------ codebook
def codebook_tables(cb):
    """The tables the library builds when it loads a codebook (K, D) fp32, in fp32 as it builds them: centre = the fp32 sum over k,
    divided by K; centred = c - centre; rnorm = 1 / max(|centred|, 1e-8) (the norm summed in double, rounded to fp32); raw = centred +
    centre.  The codebooks of these tests lie on a grid of 2^-12 with |v| < 4 and K <= 512: every partial column sum is a multiple of
    2^-12 below 2^11, exact in fp32 in any order -- asserted -- so this mirror does not depend on the library's summation order."""
    c = np.asarray(cb, dtype=np.float32)
    K, D = c.shape
    c64 = c.astype(np.float64)
    assert K <= 512 and (np.abs(c64) < 4).all() and (c64 * 4096 == np.round(c64 * 4096)).all(), "codebook off the 2^-12 grid"
    col = c64.sum(0)
    assert (np.abs(c64).sum(0) < 2048).all() and (col.astype(np.float32).astype(np.float64) == col).all()
    centre = col.astype(np.float32) / np.float32(K)
    cc = c - centre[None, :]
    norm = np.sqrt((cc.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    rnorm = np.float32(1.0) / np.maximum(norm, np.float32(1e-8))
    return dict(centre=centre, cc=cc, rnorm=rnorm, raw=cc + centre[None, :])


def _cos(p, q, mistake=None):
    """F.cosine_similarity over the last axis in float64: each norm clamped at 1e-8, then the division -> (cos, A) with
    A = sum |p q| / (the clamped norms), the factor of every bound below (A <= 1 where nothing is clamped)."""
    with np.errstate(all="ignore"):
        n1, n2 = np.sqrt((p * p).sum(-1)), np.sqrt((q * q).sum(-1))
        if mistake == "clamp_after_division":                          # the vectors divided by their raw norms: 0 / 0
            ph, qh = p / n1[..., None], q / n2[..., None]
            return (ph * qh).sum(-1), np.abs(ph * qh).sum(-1)
        den = np.maximum(n1, 1e-8) * np.maximum(n2, 1e-8)
        return (p * q).sum(-1) / den, np.abs(p * q).sum(-1) / den


def codebook_frame(v, tables, target, mistake=None):
    """v (F, D) fp32 feature rows, target (F) labels in [0, K) -> float64 dict(cos (F, K) against every centred centroid, pred = their
    arg-max by the rule, term = 1 - cos(v, c_target), cos_pt = cos(c_pred, c_target)) and the fp32 bounds:
      amax (F): g(D + 3) max_k A_k on a cosine as the arg-max sees it -- a D-long fma chain, the rounding of the centroid's norm to
        fp32, its reciprocal, and the product with it (|v| is common to all k and is not divided by);
      term, cos_pt (F): g(20) A [+ u |term| for the rounding of 1 - cos] -- each norm is a square (1 rounding), a 128-wide tree (six
        shuffle adds in a wave, one add of the two waves: 7) and a sqrt, which halves those 8 and adds 1 (5 per norm, 10 for two);
        then two divisions (2), the product (1) and another 128-wide tree (7): n = 20."""
    v64, cc = f64(v), f64(tables["cc"])
    D = v64.shape[1]
    cos, A = _cos(v64[:, None, :], cc[None, :, :], mistake)
    pred = argmax_rule(cos, mistake)
    F = np.arange(len(pred))
    tgt = np.asarray(target)
    term = 1.0 - cos[F, tgt]
    cos_pt, A_pt = _cos(cc[np.minimum(pred, len(cc) - 1)], cc[tgt], mistake)
    with np.errstate(all="ignore"):
        return dict(cos=cos, pred=pred, term=term, cos_pt=cos_pt, amax=g(D + 3) * A.max(1), bound_term=g(20) * A[F, tgt] + U * np.abs(term),
                    bound_pt=g(20) * A_pt)


def cos_pt_of(tables, pred, target):
    """cos(c_pred, c_target) in float64 and its bound, for the labels a kernel returned."""
    cc = f64(tables["cc"])
    c, A = _cos(cc[np.asarray(pred)], cc[np.asarray(target)])
    return c, g(20) * A


def _grid(v):
    """v on the grid of 2^-12, clipped to |v| <= 15974 / 4096 < 4."""
    return (np.clip(np.round(np.asarray(v) * 4096), -15974, 15974) / 4096).astype(np.float32)


def grid_codebook(K, D, rng):
    return _grid(rng.standard_normal((K, D)))


CODEBOOK_PAIRS = ((7, 135), (9, 10), (20, 84), (21, -1), (0, 1))        # one thread (k, k + 128) | neighbouring lanes | the two waves | to K - 1
CODEBOOK_DUPS = ((5, 6), (5, 70), (5, 133))


def codebook_case(K, D, seed=0, members=24):
    """A grid-quantised codebook (K, D) with duplicate rows at CODEBOOK_DUPS and, for every near-tie pair, b = a + 0.5 N(0, 1); feature
    rows (F, D): noisy members of known centroids, members of the duplicated centroid 5 (label 5), for every pair two near-tie rows (a
    wins, b wins) whose cosine gap is 8 times the larger of the two arg-max bounds, a zero row and a NaN row (label 0 both).  At D = 1
    every cosine is +-1 and all centroids of a sign tie: no near-tie rows, and the arg-max is held to the tie set (codebook_check).
    -> dict(cb, tables, v fp32 (F, D), kind (F) of "member" / "dup" / "near" / "zero" / "nan", want (F) or -1, target (F))."""
    rng = np.random.default_rng(77 * seed + 1000 * K + D)
    cb = grid_codebook(K, D, rng)
    pairs = _pairs(K, [(a, b if b >= 0 else K + b) for a, b in CODEBOOK_PAIRS]) if D > 1 else []
    for a, b in pairs:
        cb[b] = _grid(cb[a] + 0.5 * rng.standard_normal(D))
    dups = [(a, b) for a, b in CODEBOOK_DUPS if b < K]
    for a, b in dups:
        cb[b] = cb[a]
    tables = codebook_tables(cb)
    cc = f64(tables["cc"])
    rows, kind, want = [], [], []
    for k in rng.integers(0, K, members):
        rows.append(cc[k] + 0.3 * rng.standard_normal(D)); kind.append("member"); want.append(-1)
    for _ in range(3 if dups else 0):
        rows.append(cc[5] + 0.05 * rng.standard_normal(D)); kind.append("dup"); want.append(5 if D > 1 else -1)
    for a, b in pairs:
        for a, b in ((a, b), (b, a)):                                  # a wins, then b wins
            ah, bh = cc[a] / np.linalg.norm(cc[a]), cc[b] / np.linalg.norm(cc[b])
            base = ah + bh
            if np.linalg.norm(base) < 1e-3:                            # K = 2: the centred pair is c, -c; any row orthogonal to it ties
                base = rng.standard_normal(D)
                base -= (base @ ah) * ah
            row = base
            for _ in range(3):
                fr = codebook_frame(row[None].astype(np.float32), dict(cc=tables["cc"][[a, b]]), [0])
                t = 8.0 * fr["amax"][0] * np.linalg.norm(row) / (2.0 * (1.0 - ah @ bh))
                row = base + t * (ah - bh)                              # (row . ah - row . bh) / |row| = 2 t (1 - ah . bh) / |row|
            rows.append(3.0 * row); kind.append("near"); want.append(a)
    rows.append(np.zeros(D)); kind.append("zero"); want.append(0)
    rows.append(np.where(np.arange(D) == D // 2, np.nan, 1.0)); kind.append("nan"); want.append(0)
    v = np.asarray(rows).astype(np.float32)
    target = rng.integers(0, K, len(v))
    return dict(cb=cb, tables=tables, v=v, kind=np.asarray(kind), want=np.asarray(want), target=target, K=K, D=D)


def codebook_check(case, pred, terms, cos_pt):
    """Hold a kernel's per-frame outputs to the float64 definition on a codebook_case.  Every row: the cosine of the kernel's label is
    within twice the arg-max bound of the largest (so it IS the float64 arg-max wherever the gap exceeds that: every member, dup and
    near-tie row at D > 1, asserted; zero and NaN rows get label 0; near-tie gaps lie between 3 and 10 times twice the bound),
    terms and cos_pt within their bounds.  -> max err / bound over (near, dup, zero and NaN rows | members)."""
    fr = codebook_frame(case["v"], case["tables"], case["target"])
    kind, want, D = case["kind"], case["want"], case["D"]
    w, gap = winner_gap(fr["cos"], case["tables"]["cc"], -1.0)
    assert (w == fr["pred"]).all()
    finite = ~np.isin(kind, ("zero", "nan"))
    if D > 1:
        assert (gap[finite] > 2 * fr["amax"][finite]).all(), ("rows that are no clear win", np.nonzero(finite & (gap <= 2 * fr["amax"]))[0])
        ratio = gap[kind == "near"] / (2 * fr["amax"][kind == "near"])
        assert ((ratio >= 3) & (ratio <= 10)).all(), ratio
    assert (w[want >= 0] == want[want >= 0]).all(), (w[want >= 0], want[want >= 0])
    pred, terms, cos_pt = np.asarray(pred), np.asarray(terms, dtype=np.float64), np.asarray(cos_pt, dtype=np.float64)
    assert ((pred >= 0) & (pred < case["K"])).all(), pred
    F = np.arange(len(pred))
    if D > 1:
        assert (pred == w).all(), ("pred", np.nonzero(pred != w)[0], pred[pred != w], w[pred != w])
    else:                                                              # every centroid of the row's sign ties: the label is one of them
        assert (pred[~finite] == 0).all() and (fr["cos"][F, pred][finite] >= fr["cos"][F, w][finite] - 2 * fr["amax"][finite]).all()
    cpt, bound_pt = cos_pt_of(case["tables"], pred, case["target"])
    nan = kind == "nan"
    assert np.isnan(terms[nan]).all() and np.isnan(fr["term"][nan]).all() and np.isfinite(terms[~nan]).all() and np.isfinite(cos_pt).all()
    q = np.zeros(len(pred))
    for err, bound in ((np.abs(terms - fr["term"]), fr["bound_term"]), (np.abs(cos_pt - cpt), bound_pt)):
        ok = ~nan
        assert (err[ok & (bound == 0)] == 0).all()                     # a zero row: every product is an exact 0
        q[ok & (bound > 0)] = np.maximum(q[ok & (bound > 0)], (err / np.where(bound > 0, bound, 1.0))[ok & (bound > 0)])
    assert (q <= 1).all(), ("terms / cos_pt: err / bound", np.nonzero(q > 1)[0], q.max())
    edge = kind != "member"
    return float(q[edge].max(initial=0.0)), float(q[~edge].max(initial=0.0))


# ------------------------------------------------------------------------------------------------------------ the unit splice
def code_splice(clean, masked, first, last, mistake=None):
    """(B, T) unit series and per-clip frames -> the script's two slice assignments: `out = masked; out[:first] = clean[:first];
    out[last:] = clean[last:]` (a negative `first` or `last` is the kernel's plain comparison `t < first || t >= last`, not Python's
    count from the end: the engine never passes one)."""
    clean, masked = np.asarray(clean), np.asarray(masked)
    out = masked.copy()
    T = clean.shape[1]
    for b in range(clean.shape[0]):
        f, l = int(first[b]), int(last[b])
        if mistake == "splice_off_by_one":
            f, l = f + 1, l + 1
        f, l = min(max(f, 0), T), min(max(l, 0), T)
        out[b, :f] = clean[b, :f]
        out[b, l:] = clean[b, l:]
    return out


# ------------------------------------------------------------------------------------------------------------ mel metrics, SI-SDR
def mel_metrics(a, b, center=None, mistake=None):
    """a, b (D, L) fp32 mel segments, center (D) or None -> float64 (avg_cosine_sim, avg_d2_dist, rmse) by the statements of
    ref_cpu.mel_signal_metrics, and their fp32 bounds (3).

    Cosine: per frame g(D + 3) A_l with A_l = sum |(x - c)(y - c)| / (the clamped norms): the D-long fma chain of the dot, the sqrt,
    the product of the norms and the division.  (This is the count the pin was specified with, and the tighter one: a strict worst
    case also adds the norms' own chains, at half weight through the sqrt, and the two subtractions of c, once each: 2 D + 8.  The
    kernel is held to D + 3.)  The mean over frames is summed in double; u |value| for the store.
    The two dB values, first order in u except where marked: the bin mean m is D - 1 adds and a division, |dm| <= g(D) mean|x|;
    e_d = (x_d - ma) - (y_d - mb) is three roundings of exact differences, |de_d| <= dma + dmb + u (|x_d - ma| + |y_d - mb| + |e_d|);
    sq = sum e^2 is a D-long fma chain, |dsq| <= sum (2 |e_d| |de_d| + de_d^2) + g(D + 1) sum e^2 (the square of de is kept: where
    e = 0 it is all there is); sqrt(sq / D) adds a division and a sqrt, and |sqrt(p + d) - sqrt(p)| <= min(sqrt |d|, |d| / sqrt p);
    the sums over frames are in double; u |value| for the store."""
    x, y = f64(a), f64(b)
    D, L = x.shape
    c = np.zeros(D) if center is None else f64(center)
    cos, A = _cos((x - c[:, None]).T, (y - c[:, None]).T, mistake)
    cos_v = cos.mean()
    ax = 1 if mistake == "mean_over_frames" else 0
    ma, mb = x.mean(ax, keepdims=True), y.mean(ax, keepdims=True)
    e = (x - ma) - (y - mb)
    sq = (e * e).sum(0)
    d2_l = np.sqrt(sq / D)
    d2_v, rmse_v = LOG_SCALE * d2_l.mean(), LOG_SCALE * np.sqrt(sq.sum() / (D * L))
    # bounds
    b_cos = g(D + 3) * A.mean() + U * abs(cos_v)
    dm = g(D) * (np.abs(x).mean(0) + np.abs(y).mean(0))
    de = dm[None, :] + U * (np.abs(x - ma) + np.abs(y - mb) + np.abs(e))
    dsq = (2 * np.abs(e) * de + de * de).sum(0) + g(D + 1) * sq
    def dsqrt(p, d):
        with np.errstate(all="ignore"):
            return np.where(p > 0, np.minimum(np.sqrt(d), d / np.sqrt(np.where(p > 0, p, 1.0))), np.sqrt(d)) + 2 * U * np.sqrt(p)
    b_d2 = LOG_SCALE * dsqrt(sq / D, dsq / D).mean() + U * abs(d2_v)
    b_rmse = LOG_SCALE * float(dsqrt(sq.sum() / (D * L), dsq.sum() / (D * L))) + U * abs(rmse_v)
    return np.array([cos_v, d2_v, rmse_v]), np.array([b_cos, b_d2, b_rmse])


EPS32 = 2.0 ** -23


def sisdr(est, ref):
    """est, ref (n) fp32 -> float64 (SI-SDR in dB, its bound) by the statements of ref_cpu.sisdr with eps = 2^-23: a = (eps + ref.est)
    / (|ref|^2 + eps), value = 10 log10((eps + |a ref|^2) / (eps + |est - a ref|^2)), the residual computed directly (stable).  The
    kernel expands it as ee - 2 a re + a^2 rr from three n-long double sums, which cancels: d = 8 n 2^-53 (ee + 2 |a re| + a^2 rr)
    bounds that, the log turns d / (eps + snn) into (10 / ln 10) of it in dB, and the store to fp32 adds 2^-23 |value|."""
    e, r = f64(est), f64(ref)
    n = e.size
    rr, re, ee = r @ r, r @ e, e @ e
    a = (EPS32 + re) / (rr + EPS32)
    sss, snn = ((a * r) ** 2).sum(), ((e - a * r) ** 2).sum()
    val = 10.0 * np.log10((EPS32 + sss) / (EPS32 + snn))
    d = 8 * n * 2.0 ** -53 * (ee + 2 * abs(a * re) + a * a * rr)
    return val, (10.0 / np.log(10.0)) * d / (EPS32 + snn) + 2.0 ** -23 * abs(val)


def per_clip(fn, *batched, mistake=None):
    """fn applied to each clip of the batched arguments (leading axis), stacked; `clip_zero`: every clip reads clip 0."""
    B = len(batched[0])
    return [fn(*[arg[0 if mistake == "clip_zero" else i] for arg in batched]) for i in range(B)]


def mel_case(D, L, seed=0):
    """Three different clips (3, D, L) on a grid of 2^-10, and the three edge pairs: identical inputs; a pair whose second clip is the
    first plus an offset per frame (constant over the bins: the bin mean removes it exactly); a pair whose first clip has one frame
    equal to `center`.  -> dict(a, b (3, D, L), center (D), edges {name: (a, b) (D, L)})."""
    rng = np.random.default_rng(31 * seed + 1000 * D + L)
    q = lambda v: (np.round(v * 1024) / 1024).astype(np.float32)
    a = q(rng.standard_normal((3, D, L)) * np.array([1.0, 2.0, 0.5])[:, None, None] - 5.0)
    b = q(a + rng.standard_normal((3, D, L)) * np.array([0.3, 0.05, 1.0])[:, None, None])
    center = q(-5.0 + 0.2 * rng.standard_normal(D))
    off = q(a[0] + np.round(rng.standard_normal(L) * 4)[None, :] / 4)
    zero = a[2].copy()
    zero[:, L // 2] = center
    return dict(a=a, b=b, center=center, edges={"identical": (a[1], a[1].copy()), "offset": (a[0], off), "zero_norm": (zero, b[2])})


def sisdr_case(n, seed=0):
    """ref (3, n): three different clips with values 10 m 2^-16, |m| <= 3000, so that 0.7 ref is representable; noise (3, n)."""
    rng = np.random.default_rng(17 * seed + n)
    ref = (10.0 * rng.integers(-3000, 3001, (3, n)) / 65536.0) * np.array([1.0, 0.5, 0.25])[:, None]
    noise = rng.standard_normal((3, n))
    assert (f64(0.7 * ref) * 10 == 7 * f64(ref)).all()                 # est = 0.7 ref holds exactly in fp32
    return ref.astype(np.float32), noise


# ------------------------------------------------------------------------------------------------------------ the cases of the GPU tests
# rows x D x K.  D % 32 == 0 runs on the MFMA kernel unless SI_KMEANS_MFMA=0; 80 is the scalar kernel on both settings.
KMEANS_SHAPES = {
    (1, 32, 1): "one row, one centroid, one trip of the MFMA kernel's D loop",
    (31, 32, 2): "fewer rows than a tile (clamped loads), K below a column tile",
    (32, 64, 127): "exactly one row tile, K one short of the 128-centroid block",
    (33, 64, 128): "a second tile of one row, K exactly one block",
    (65, 96, 129): "three tiles, D = 96 (three trips per lane half), one centroid in the second block",
    (40, 256, 256): "K exactly two blocks",
    (40, 256, 257): "one centroid in a third block",
    (7, 80, 3): "the scalar kernel (D % 32 != 0), K below a wave",
    (300, 80, 300): "the scalar kernel past its 256-thread stride",
}
CODEBOOK_SHAPES = ((1, 80), (2, 80), (63, 80), (64, 80), (65, 80), (127, 80), (128, 80), (129, 80), (257, 80), (500, 80), (100, 1),
                   (100, 64), (100, 65), (100, 128))                    # K x D: around the wave (64) and the 128 threads; D up to the limit
SPLICE_KS = (1, 129, 500)
MEL_SHAPES = tuple((D, L) for D in (80, 1) for L in (1, 255, 256, 257, 513))      # L around the 256-thread stride
SISDR_NS = (1, 63, 64, 1023, 1024, 1025, 4099)                        # around the wave and the 1024-thread stride
SISDR_NOISE = (0.5, 1e-2, 1e-4, 0.0)
SPLICE_TS = (1, 255, 256, 257)


def kmeans_dup_case(D, K, dup, seed=0):
    """Centroid `dup` is a copy of centroid 3 (all of KMEANS_DUPS that fit when dup is None); 33 members of that cluster: label 3."""
    rng = np.random.default_rng(5 * seed + 100 * D + K)
    cent = rng.standard_normal((K, D)).astype(np.float32)
    for a, b in KMEANS_DUPS:
        if b < K and dup in (None, b):
            cent[b] = cent[a]
    x = (cent[3][None, :] + 0.3 * rng.standard_normal((33, D))).astype(np.float32)
    return dict(x=x, cent=cent, near=np.zeros(33, bool), edge=np.ones(33, bool), want=np.full(33, 3, np.int64))


NONFINITE_ROWS = {5: "one NaN", 6: "all NaN", 17: "+inf", 19: "1e30", 34: "3e38"}


def kmeans_nonfinite_case(D, K, seed=0):
    """kmeans_case(40, D, K) with rows 5 (one NaN), 6 (all NaN), 17 (+inf), 19 (1e30: |x|^2 overflows) and 34 (3e38: the products of
    the dot overflow) replaced: rows 5 and 6 get label 0, the others some label in [0, K), and the finite rows -- the neighbours in
    the first 32-row tile are its near-tie rows -- keep their float64 labels.  `finite` marks those."""
    case = kmeans_case(40, D, K, seed)
    x = case["x"]
    x[5, D // 3] = np.nan
    x[6], x[17], x[19], x[34] = np.nan, np.inf, 1e30, 3e38
    case["finite"] = ~np.isin(np.arange(40), list(NONFINITE_ROWS))
    case["want"][~case["finite"]] = -1
    case["near"] &= case["finite"]
    return case


def kmeans_nonfinite_check(case, labels, dist):
    labels = np.asarray(labels)
    K = len(case["cent"])
    assert ((labels >= 0) & (labels < K)).all(), ("out of range", labels[(labels < 0) | (labels >= K)])
    assert labels[5] == 0 and labels[6] == 0, labels[[5, 6]]
    return kmeans_check(case, labels, dist)


def code_splice_ranges(T):
    """(first, last) per clip, two launches of B = 3: empty, whole, first > last | last > T, first < 0, interior."""
    return [[(T // 2, T // 2), (0, T), (min(T, 3), min(T, 3) - 1)], [(T // 2, T + 5), (-3, T // 2 + 1), (T // 3, 2 * T // 3 + 1)]]
