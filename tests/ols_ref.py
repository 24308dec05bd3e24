"""Host references for the edge tests of the small regression and row-set kernels (test
infrastructure, CPU only): tests/test_solve_edges_gpu.py, tests/test_predict_fm_gpu.py,
tests/test_rowsets_gpu.py and their CPU checks in tests/test_ols_ref.py.

* ``moments``: the (gram, shift) of [1, x, y] in the three representations ``afm_ols_solve_f64``
  meets, summed in ``np.longdouble`` and rounded once to fp64.
* ``ols_kept``: longdouble least squares (Householder QR of the centered, unit-scaled design) on
  a chosen set of columns; ``scaled_pivots`` / ``cond_scaled``: where a design sits relative to the
  solver's ``tol`` and to the accuracy bar.
* ``predict_seq``, ``residual_seq``, ``intercept_seq``, ``fm_ref``, ``labels_ref``,
  ``drop_last_ref``, ``row_bits_ref``: the documented operation order of the kernels restated in
  fp64 / Python-int arithmetic (compared bit for bit), plus the designs the GPU tests share.
"""
import numpy as np

LD = np.longdouble
KINDS = ("first", "pooled", "raw")
COND_CAP = 300.0          # cond^2 * 2^-53 * 10 <= 1e-10: a tenth of the 1e-9 accuracy bar
NAN_BITS = 0x7FF8000000000000       # the quiet NaN the kernels write (__builtin_nan(""))


# ---- moments ------------------------------------------------------------------------------------
def moments(X, y, kind):
    """-> (gram [p+2][p+2], shift [p+2]) of Z = [1, x, y] over the rows of X [n][p], y [n].

    gram = sum (z - shift)(z - shift)^T with column 0 unshifted, so gram[0][0] = n and gram[0][j] =
    sum (z_j - shift_j).  ``first``: shift = the first row (afm_xs_gram_f64); ``pooled``: shift = the
    means, row / column 0 = n, 0... (pool_kernel); ``raw``: shift = 0 (afm_gram_tree_f64 final
    output).  No rows: all zeros (the Gram kernel's n = 0 segment)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = X.shape
    G = np.zeros((p + 2, p + 2))
    s = np.zeros(p + 2)
    if n == 0:
        return G, s
    Z = np.concatenate([X, y[:, None]], axis=1).astype(LD)
    if kind == "first":
        sh = Z[0].copy()
    elif kind == "pooled":
        sh = Z.sum(axis=0) / LD(n)
    elif kind == "raw":
        sh = np.zeros(p + 1, dtype=LD)
    else:
        raise ValueError(kind)
    sh64 = sh.astype(np.float64)                     # the shift the solver adds back
    D = Z - sh64.astype(LD)
    G[0, 0] = n
    if kind != "pooled":
        G[0, 1:] = G[1:, 0] = D.sum(axis=0).astype(np.float64)
        G[1:, 1:] = (D.T @ D).astype(np.float64)
    else:                                            # centered sums; row 0 is exactly n, 0...
        Dc = Z - sh
        G[1:, 1:] = (Dc.T @ Dc).astype(np.float64)
    s[1:] = sh64
    return G, s


def centered_moments(G, s):
    """(gram, shift) -> (n, mean [p+1], C [p+1][p+1]) in longdouble: what every kind describes."""
    G = np.asarray(G).astype(LD)
    n = G[0, 0]
    m = G[0, 1:] / n
    C = G[1:, 1:] - np.outer(G[0, 1:], G[0, 1:]) / n
    return n, np.asarray(s).astype(LD)[1:] + m, C


# ---- longdouble least squares -------------------------------------------------------------------
def _center_scale(X):
    X = np.asarray(X, dtype=np.float64).astype(LD)
    xm = X.sum(axis=0) / LD(X.shape[0])
    Xc = X - xm
    nrm = np.sqrt((Xc * Xc).sum(axis=0))
    return Xc, xm, nrm


def _householder_lstsq(A, b):
    """min ||A w - b|| for a full-column-rank longdouble A [n][k], by Householder QR."""
    A, b = A.copy(), b.copy()
    n, k = A.shape
    for j in range(k):
        x = A[j:, j]
        nrm = np.sqrt(x @ x)
        v = x.copy()
        v[0] += nrm if x[0] >= 0 else -nrm
        vv = v @ v
        if vv == 0:
            continue
        f = LD(2) / vv
        A[j:, j:] -= np.outer(v, f * (v @ A[j:, j:]))
        b[j:] -= v * (f * (v @ b[j:]))
    w = np.zeros(k, dtype=LD)
    for j in range(k - 1, -1, -1):
        w[j] = (b[j] - A[j, j + 1:k] @ w[j + 1:]) / A[j, j]
    return w


def ols_kept(X, y, kept):
    """Longdouble OLS of y on [1, X[:, kept]] -> beta [p+1] (longdouble): intercept first, the
    coefficients of the columns outside ``kept`` exactly 0.0, intercept = ybar - xbar . b."""
    X = np.asarray(X, dtype=np.float64)
    p = X.shape[1]
    kept = np.asarray(kept, dtype=np.int64)
    y = np.asarray(y, dtype=np.float64).astype(LD)
    ym = y.sum() / LD(len(y))
    beta = np.zeros(p + 1, dtype=LD)
    if len(kept):
        Xc, xm, nrm = _center_scale(X[:, kept])
        w = _householder_lstsq(Xc / nrm, y - ym) / nrm
        beta[1 + kept] = w
        beta[0] = ym - xm @ w
    else:
        beta[0] = ym
    return beta


def scaled_pivots(X, drop_below=0.0):
    """The pivots of the right-looking Cholesky of the centered, unit-diagonal moments of X in
    column order (longdouble): what ``afm_ols_solve_f64`` compares with ``tol``.  A column whose
    pivot is <= drop_below is not eliminated (a dropped regressor)."""
    Xc, _, nrm = _center_scale(X)
    ok = nrm > 0
    Xs = np.where(ok, Xc / np.where(ok, nrm, LD(1)), LD(0))
    M = Xs.T @ Xs
    p = M.shape[0]
    piv = np.zeros(p, dtype=LD)
    for k in range(p):
        piv[k] = M[k, k]
        if piv[k] > drop_below:
            M[k + 1:, k + 1:] -= np.outer(M[k + 1:, k], M[k + 1:, k]) / piv[k]
    return piv


def cond_scaled(X):
    """2-norm condition number of the centered, unit-scaled design."""
    Xc, _, nrm = _center_scale(X)
    sv = np.linalg.svd((Xc / nrm).astype(np.float64), compute_uv=False)
    return float(sv[0] / sv[-1])


def rel_err(got, ref):
    """The project's accuracy figure: max |b - ref| / max |ref|."""
    ref = np.asarray(ref).astype(LD)
    return float(np.abs(np.asarray(got).astype(LD) - ref).max() / np.abs(ref).max())


# ---- the designs of tests/test_solve_edges_gpu.py -----------------------------------------------
FULL_P = (1, 15, 16, 17, 63, 64, 65, 110)
UNDER_P = (5, 70)
DEFICIENT_P = (6, 70)
DEFICIENT_CASES = ("duplicate", "duplicate_hi", "combination", "combination_hi", "const_first",
                   "const_middle", "const_last", "const_all")
OFFSET_P = (3, 30)
OFFSET_RATIOS = (1.0, 1e2, 1e4, 1e6)
TOL_P = (6, 70)
TOL_KEEP, TOL_DROP = 1e-10, 1e-4


def _gauss_design(rng, n, p, scales=True):
    X = rng.normal(size=(n, p))
    if scales:                                       # column scales spread over 1e-6 .. 1e6
        e = np.linspace(-6.0, 6.0, p) if p > 1 else np.array([3.0])
        X = X * 10.0 ** rng.permutation(e)
    b = rng.normal(size=p) / np.abs(X).mean(axis=0) if n else np.zeros(p)
    y = X @ b + 0.3 * rng.normal(size=n) + 2.0
    return X, y


def full_rank_design(p, n):
    """Gaussian columns with scales over 1e-6 .. 1e6, mean/sd < 1.  (Square centered designs,
    n = p + 1, are often ill-conditioned: tests/test_ols_ref.py asserts the cap for these seeds.)"""
    return _gauss_design(np.random.default_rng([11, p, n]), n, p)


def full_rank_cases():
    out = []
    for p in FULL_P:
        out.append((p, 2 * p + 5))
        if p <= 17:
            out.append((p, p + 1))
    return out


def under_determined_ns(p):
    """The nine segments of one launch: n <= p gives NaN, n > p is solved."""
    return [2 * p + 5, 0, 1, p + 1, p - 1, p, 2 * p + 5, 0, p + 1]


def under_determined_design(p, k):
    n = under_determined_ns(p)[k]
    return _gauss_design(np.random.default_rng([13, p, k]), n, p)


def deficient_design(p, case):
    """-> (X, y, kept): a rank-deficient design and the columns a first-occurrence rule keeps.
    ``_hi`` cases put the dependent column at an index >= 64 (p = 70 only; at p = 6 they use the
    last column)."""
    n = 2 * p + 5
    rng = np.random.default_rng([17, p, DEFICIENT_CASES.index(case)])
    X, _ = _gauss_design(rng, n, p)
    lo, hi = (2, p - 1) if p < 64 else (40, 66)
    drop = []
    if case in ("duplicate", "duplicate_hi"):
        j = lo if case == "duplicate" else hi
        X[:, j] = X[:, 1]
        drop = [j]
    elif case in ("combination", "combination_hi"):
        j = lo if case == "combination" else hi
        # multiples of 1/8 and power-of-two weights: the combination is exact in fp64
        X[:, 0] = rng.integers(-1000, 1001, size=n) / 8.0
        X[:, 1] = rng.integers(-1000, 1001, size=n) / 8.0
        X[:, j] = 0.5 * X[:, 0] - 2.0 * X[:, 1]
        drop = [j]
    elif case in ("const_first", "const_middle", "const_last"):
        j = {"const_first": 0, "const_middle": p // 2 if p < 64 else 64, "const_last": p - 1}[case]
        X[:, j] = {"const_first": 37.3, "const_middle": -12.7, "const_last": 0.017}[case]
        drop = [j]
    elif case == "const_all":
        X[:] = rng.uniform(-50.0, 50.0, size=p)
        drop = list(range(p))
    else:
        raise ValueError(case)
    kept = np.array([j for j in range(p) if j not in drop], dtype=np.int64)
    b = np.zeros(p)
    if len(kept):
        b[kept] = rng.normal(size=len(kept)) / np.abs(X[:, kept]).mean(axis=0)
    y = X @ b + 0.3 * rng.normal(size=n) + 2.0
    return X, y, kept


def tol_design(p):
    """-> (X, y, j): column j = column 1 + delta * independent noise, delta placed so that its
    scaled pivot is about 1e-6: kept at tol = 1e-10, dropped at tol = 1e-4."""
    n = 2 * p + 5
    rng = np.random.default_rng([19, p])
    X, _ = _gauss_design(rng, n, p, scales=False)
    j = p - 2 if p < 64 else 66
    X[:, j] = X[:, 1] + 5e-4 * rng.normal(size=n)
    y = X @ rng.normal(size=p) + 0.3 * rng.normal(size=n) + 2.0
    return X, y, j


def offset_design(p, ratio):
    """Unit-variance columns with mean = ratio * sd (signs alternate), n = 200."""
    n = 200
    rng = np.random.default_rng([23, p])
    X = rng.normal(size=(n, p))
    X = (X - X.mean(axis=0)) / X.std(axis=0)
    y = X @ rng.normal(size=p) + 0.3 * rng.normal(size=n) + 2.0
    return X + ratio * np.where(np.arange(p) % 2, -1.0, 1.0), y


def raw_variance_fp64(G, r):
    """d = G[r][r] - G[0][r]^2 / n in fp64, as the solver forms it."""
    return G[r, r] - G[0, r] * G[0, r] / G[0, 0]


# ---- sequential fp64 restatements ---------------------------------------------------------------
def predict_seq(b, x):
    """s = b[0]; s = s + b[1 + j] * x[j], j ascending.  b [..., p+1] broadcasts against
    x [p][...]."""
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        s = b[..., 0] + np.zeros(x.shape[1:])
        for j in range(x.shape[0]):
            t = b[..., 1 + j] * x[j]
            s = s + t
    return s


def predict_ld(b, x):
    """(longdouble dot product, sum of |terms|) of the same prediction."""
    b = np.asarray(b).astype(LD)
    with np.errstate(all="ignore"):
        s = b[..., 0] + np.zeros(x.shape[1:], dtype=LD)
        mag = np.abs(s)
        for j in range(x.shape[0]):
            t = b[..., 1 + j] * x[j].astype(LD)
            s = s + t
            mag = mag + np.abs(t)
    return s, mag


def residual_seq(Z, p, ycol, mean, beta):
    """s = Z[ycol] - mean[p+1]; s = s - beta[1+j] * (Z[j] - mean[1+j]), j ascending."""
    s = Z[ycol] - mean[p + 1]
    for j in range(p):
        d = Z[j] - mean[1 + j]
        t = beta[1 + j] * d
        s = s - t
    return s


def intercept_seq(p, mean, beta):
    """icpt = mean[p+1]; icpt = icpt - mean[1+j] * beta[1+j], j ascending."""
    icpt = np.float64(mean[p + 1])
    for j in range(p):
        t = np.float64(mean[1 + j]) * np.float64(beta[1 + j])
        icpt = icpt - t
    return icpt


def fm_ref(beta, rank):
    """Longdouble Fama-MacBeth over the rows with rank > 0 -> (mean [k], t [k]) as fp64: mean and
    mean / (std(ddof=1) / sqrt(n)); no usable row -> NaN, NaN; one -> t NaN."""
    use = np.asarray(rank) > 0
    B = np.asarray(beta)[use].astype(LD)
    n, k = B.shape
    nan = np.full(k, np.nan)
    if n == 0:
        return nan, nan
    m = B.sum(axis=0) / LD(n)
    if n == 1:
        return m.astype(np.float64), nan
    sd = np.sqrt(((B - m) ** 2).sum(axis=0) / LD(n - 1))
    with np.errstate(all="ignore"):
        t = m / (sd / np.sqrt(LD(n)))
    return m.astype(np.float64), t.astype(np.float64)


# ---- row sets -----------------------------------------------------------------------------------
PATTERNS = ("never", "single", "day0", "last_day", "word_edge", "far_apart", "dense", "random")


def presence(T, lda, A, seed=0):
    """[T][lda] bool: asset a < A follows PATTERNS[a % 8] (patterns a short T cannot hold are
    never present); the pad columns A..lda are never present."""
    rng = np.random.default_rng([29, T, lda, seed])
    v = np.zeros((T, lda), dtype=bool)
    for a in range(A):
        k = PATTERNS[a % len(PATTERNS)]
        if k == "single":
            v[rng.integers(0, T), a] = True
        elif k == "day0":
            v[0, a] = True
        elif k == "last_day":
            v[T - 1, a] = True
        elif k == "word_edge" and T > 64:
            v[63, a] = v[64, a] = True
        elif k == "far_apart" and T >= 200:          # words 0 and 3, words 1-2 empty
            v[rng.integers(0, 64), a] = v[rng.integers(192, T), a] = True
        elif k == "dense":
            v[:, a] = True
        elif k == "random":
            v[:, a] = rng.random(T) < 0.5
    return v


def pack_words(v):
    """[T][lda] bool -> [ceil(T/64)][lda] uint64 presence words (bit s of word c = day 64c + s)."""
    T, lda = v.shape
    nch = (T + 63) // 64
    pad = np.zeros((nch * 64, lda), dtype=np.uint64)
    pad[:T] = v
    sh = np.arange(64, dtype=np.uint64).reshape(1, 64, 1)
    return (pad.reshape(nch, 64, lda) << sh).sum(axis=1, dtype=np.uint64)


def labels_ref(excess, ret1d, v, t0, t1, target, tmr):
    """Per asset shift(-1) over its present days: the present cells of the dates [t0, t1) (clamped
    to [0, T)) of ``target`` / ``tmr`` take the next present day's excess / ret1d, NaN on the
    asset's last present day; every other cell is left as it is.  Returns copies."""
    T, lda = v.shape
    target, tmr = target.copy(), tmr.copy()
    t0, t1 = max(t0, 0), min(t1, T)
    for a in range(lda):
        days = np.flatnonzero(v[:, a])
        for i, t in enumerate(days):
            if t0 <= t < t1:
                last = i + 1 == len(days)
                target[t, a] = np.nan if last else excess[days[i + 1], a]
                tmr[t, a] = np.nan if last else ret1d[days[i + 1], a]
    return target, tmr


def drop_last_ref(vwords, in_words, out_words, c0, c1):
    """Words [c0, c1) of ``out_words`` = ``in_words`` without the bit of the asset's last present
    day (taken from every word of ``vwords``); other words unchanged.  Python-int arithmetic."""
    nch, lda = vwords.shape
    out = out_words.copy()
    for a in range(lda):
        whole = 0
        for c in range(nch):
            whole |= int(vwords[c, a]) << (64 * c)
        last = whole.bit_length() - 1                # -1: never present
        for c in range(c0, c1):
            w = int(in_words[c, a])
            if last >= 0 and last >> 6 == c:
                w &= ~(1 << (last & 63))
            out[c, a] = w
    return out


def row_bits_ref(a, b, asset_ok, t0, t1):
    """out[c][i] = a & b (optional) & (asset_ok[i] ? ~0 : 0) (optional), days outside [t0, t1)
    cleared.  Python-int arithmetic."""
    nch, lda = a.shape
    out = np.zeros_like(a)
    for c in range(nch):
        lo, hi = max(t0 - 64 * c, 0), min(t1 - 64 * c, 64)
        mask = ((1 << hi) - 1) & ~((1 << lo) - 1) if hi > lo else 0
        for i in range(lda):
            w = int(a[c, i]) & mask
            if b is not None:
                w &= int(b[c, i])
            if asset_ok is not None and not asset_ok[i]:
                w = 0
            out[c, i] = w
    return out
