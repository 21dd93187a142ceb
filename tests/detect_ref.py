"""Dropout detection: the numpy reference of si_quiet_runs and the case builders of tests/test_detect_host.py and
tests/test_gpu_detect.py.  A plain module, imported by name; importing it needs no GPU."""
import numpy as np

CHUNK = 2048            # DT_CHUNK of detect_kernels.hip: samples per workgroup
CARRY_TILE = 1024       # DT_TILE of detect_kernels.hip: chunks per tile of the single-workgroup carry scan
THR = {np.float32: 0.0078125, np.int16: 3.0}       # the thresholds the value builders are written for (both exact in fp32)


def quiet_mask(x, thr):
    """|x[i]| <= thr per sample, the comparison in fp32 as the kernel makes it: NaN is loud, -0.0 quiet, |-32768| taken in int32."""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        mag = np.abs(x.astype(np.int32)).astype(np.float32) if x.dtype == np.int16 else np.abs(x.astype(np.float32))
        return mag <= np.float32(thr)


def quiet_runs_ref(x, thr, min_len):
    """Every maximal run of quiet samples of at least min_len samples as int32 (start, len) rows sorted by start: pad, diff, flatnonzero."""
    q = quiet_mask(x, thr)
    d = np.diff(np.concatenate(([0], q.astype(np.int8), [0])))
    start, end = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    keep = end - start >= int(min_len)
    return np.stack([start[keep], (end - start)[keep]], axis=1).astype(np.int32).reshape(-1, 2)


def mask_of(n, runs):
    """Runs [a, b) (clipped to [0, n), empty ones dropped) -> the boolean quiet mask of n samples."""
    q = np.zeros(n, dtype=bool)
    for a, b in runs:
        q[max(a, 0):max(min(b, n), 0)] = True
    return q


def materialize(quiet, dtype, seed=0):
    """A boolean quiet mask -> samples of `dtype` that are quiet under THR[dtype] exactly where the mask says so.  Quiet samples cycle
    through 0, -0.0, +-thr exactly, a subnormal and values inside; loud ones are random with planted NaN, +-inf, the first value above
    thr (fp32) or thr + 1 and -32768 (int16)."""
    quiet = np.asarray(quiet, dtype=bool)
    n = quiet.size
    rng = np.random.default_rng(seed)
    thr = THR[dtype]
    if dtype is np.float32:
        t = np.float32(thr)
        q_vals = np.array([0.0, -0.0, t, -t, 1e-40, -1e-40, t / 2, np.nextafter(t, np.float32(0))], dtype=np.float32)
        l_vals = np.array([np.nan, np.inf, -np.inf, np.nextafter(t, np.float32(1)), -np.nextafter(t, np.float32(1))], dtype=np.float32)
        x = ((rng.random(n) * 0.9 + 0.02) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    else:
        q_vals = np.array([0, 3, -3, 1, -2], dtype=np.int16)
        l_vals = np.array([-32768, 32767, 4, -4], dtype=np.int16)
        x = (rng.integers(4, 32768, n) * rng.choice([-1, 1], n)).astype(np.int16)
    qi, li = np.flatnonzero(quiet), np.flatnonzero(~quiet)
    x[qi] = q_vals[np.arange(qi.size) % q_vals.size]
    x[li[::3]] = l_vals[np.arange(li[::3].size) % l_vals.size]        # every third loud sample is a special one
    assert np.array_equal(quiet_mask(x, thr), quiet)
    return x


SEAM_N = (1, 7, 2047, 2048, 2049, 4101, 6144)


def seam_cases(n):
    """(name, quiet mask, min_len) per case at n samples: the run placements and length edges of the chunk seams."""
    C = CHUNK
    out = [("all quiet", np.ones(n, dtype=bool), 1), ("all loud", np.zeros(n, dtype=bool), 1),
           ("all quiet, min_len n + 1", np.ones(n, dtype=bool), n + 1), ("all quiet, min_len n", np.ones(n, dtype=bool), n),
           ("alternating", np.arange(n) % 2 == 0, 1), ("alternating from 1", np.arange(n) % 2 == 1, 1),
           ("from sample 0", mask_of(n, [(0, 5)]), 1), ("reaching n", mask_of(n, [(n - 5, n)]), 1),
           ("from 0 and reaching n", mask_of(n, [(0, 3), (n - 2, n)]), 2)]
    for k in range(1, -(-n // C) + 1):
        s = k * C                                                     # the seam in front of chunk k (or the end of the last full chunk)
        out += [(f"crossing seam {s}", mask_of(n, [(s - 8, s + 12)]), 1),
                (f"ending on the last sample before {s}", mask_of(n, [(s - 48, s)]), 1),
                (f"starting on sample {s}", mask_of(n, [(s, s + 52)]), 1),
                (f"one sample each side of {s}", mask_of(n, [(s - 1, s), (s + 1, s + 2)]), 1),
                (f"one sample across {s}", mask_of(n, [(s - 1, s + 1)]), 2)]
    # whole chunks inside one run: the carry (two in a row at n = 6144, a partial last chunk that is all quiet at n = 4101)
    out += [("whole chunks inside a run from chunk 0", mask_of(n, [(C - 1, n)]), 1),
            ("whole chunks inside a run that ends early", mask_of(n, [(5, n - 3)]), 1),
            ("a run of exactly the chunks 1 ..", mask_of(n, [(C, n)]), 1)]
    # lengths min_len - 1, min_len, min_len + 1 at min_len = 5, in a chunk and across each seam
    runs, a = [], 3
    for _ in range(3):
        for l in (4, 5, 6):
            runs.append((a, a + l))
            a += l + 2
    for k in range(1, n // C + 1):
        for i, l in enumerate((4, 5, 6)):
            runs.append((k * C - 2 - 40 * i, k * C - 2 - 40 * i + l))
        runs += [(k * C - 2, k * C + 2), (k * C + 10, k * C + 15), (k * C + 100 - 3, k * C + 100 + 3)]
    runs = [(a, b) for a, b in runs if a >= 0]
    out += [("lengths 4, 5, 6 at min_len 5", mask_of(n, runs), 5), ("lengths 4, 5, 6 at min_len 1", mask_of(n, runs), 1),
            ("lengths 4, 5, 6 at min_len 7", mask_of(n, runs), 7)]
    return out


def random_mask(n, density, seed):
    """Alternating loud and quiet stretches of geometric lengths; the mean quiet length is 1 / density and so is the mean loud one
    (density 0.5: two-sample stretches; 0.002: stretches of about a quarter chunk)."""
    rng = np.random.default_rng(seed)
    q = np.zeros(n, dtype=bool)
    i, quiet = 0, bool(seed & 1)
    while i < n:
        l = int(rng.geometric(density))
        q[i:i + l] = quiet
        i, quiet = i + l, not quiet
    return q


def tile_seam_case():
    """One case longer than one tile of the carry pass: a run that spans the tile seam (chunk CARRY_TILE - 1 | CARRY_TILE) with whole
    quiet chunks on both sides of it, runs that end on either side of it, one that ends ON it, and sparse random runs everywhere."""
    seam = CARRY_TILE * CHUNK
    n = seam + 3 * CHUNK + 5
    q = random_mask(n, 0.0005, 7) & random_mask(n, 0.3, 8)
    q[seam - 3 * CHUNK - 700:seam + 2 * CHUNK + 300] = False
    q |= mask_of(n, [(seam - 2 * CHUNK - 300, seam - 2 * CHUNK - 100), (seam - CHUNK - 1000, seam + CHUNK + 200), (seam + CHUNK + 300, seam + CHUNK + 400)])
    q2 = q.copy()
    q2[seam - CHUNK - 1000:seam + CHUNK + 200] = False
    q2 |= mask_of(n, [(seam - CHUNK - 1000, seam), (seam + 1, seam + 2)])
    return n, seam, q, q2
