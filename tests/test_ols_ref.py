"""CPU checks of tests/ols_ref.py: the host references the GPU edge tests compare against, and the
conditions those tests rest on (no GPU needed).

* ``ols_kept`` agrees with ``np.linalg.lstsq`` to 1e-12 on every design used on the GPU.
* The three ``moments`` kinds describe the same centered moments.
* Every design with an accuracy assertion has ``cond_scaled <= 300`` (then cond^2 * 2^-53 * 10 <=
  1e-10, a tenth of the 1e-9 bar), and the ``tol`` designs' pivot is 100x clear of both thresholds.
* The bit-level references agree with independent restatements.
"""
import numpy as np
import pytest

import ols_ref as R


def _lstsq(X, y, kept):
    # fp64 lstsq of y on [1, x - fl(mean)], columns scaled: the subtraction is exact up to the
    # rounding of the result, the ones column absorbs the error of fl(mean), and scaling keeps
    # lstsq's own error (cond * eps) at the centered design's condition number
    kept = np.asarray(kept, dtype=np.int64)
    m = X[:, kept].mean(axis=0)
    A = np.concatenate([np.ones((len(y), 1)), X[:, kept] - m], axis=1)
    sc = np.abs(A).max(axis=0)
    w = np.linalg.lstsq(A / sc, y, rcond=None)[0] / sc
    beta = np.zeros(X.shape[1] + 1, dtype=R.LD)
    beta[0] = R.LD(w[0]) - m.astype(R.LD) @ w[1:].astype(R.LD)
    beta[1 + kept] = w[1:]
    return beta


def _accuracy_designs():
    """(label, X, y, kept) of every design whose coefficients a GPU test asserts to 1e-9."""
    out = []
    for p, n in R.full_rank_cases():
        X, y = R.full_rank_design(p, n)
        out.append((f"full p={p} n={n}", X, y, np.arange(p)))
    for p in R.UNDER_P:
        for k, n in enumerate(R.under_determined_ns(p)):
            if n > p:
                X, y = R.under_determined_design(p, k)
                out.append((f"under p={p} seg={k} n={n}", X, y, np.arange(p)))
    for p in R.DEFICIENT_P:
        for case in R.DEFICIENT_CASES:
            X, y, kept = R.deficient_design(p, case)
            out.append((f"deficient p={p} {case}", X, y, kept))
    for p in R.TOL_P:
        X, y, j = R.tol_design(p)
        out.append((f"tol p={p} dropped", X, y, np.array([c for c in range(p) if c != j])))
    for p in R.OFFSET_P:
        for ratio in R.OFFSET_RATIOS:
            X, y = R.offset_design(p, ratio)
            out.append((f"offset p={p} ratio={ratio:g}", X, y, np.arange(p)))
    return out


DESIGNS = _accuracy_designs()


@pytest.mark.parametrize("label,X,y,kept", DESIGNS, ids=[d[0] for d in DESIGNS])
def test_design_meets_condition_cap_and_ols_kept_matches_lstsq(label, X, y, kept):
    if len(kept):
        c = R.cond_scaled(X[:, kept])
        assert c <= R.COND_CAP, f"{label}: cond_scaled {c:.1f}"
    ref = R.ols_kept(X, y, kept)
    dropped = np.setdiff1d(np.arange(X.shape[1]), kept)
    assert (ref[1 + dropped] == 0.0).all()
    assert R.rel_err(_lstsq(X, y, kept), ref) < 1e-12, label


def test_offset_designs_share_one_centered_solution():
    """The offset moves only the intercept: the slopes at mean/sd = 1e6 are those at 1 to the
    precision the stored columns allow (1e6 * 2^-53 per entry)."""
    for p in R.OFFSET_P:
        X1, y = R.offset_design(p, 1.0)
        X6, _ = R.offset_design(p, 1e6)
        b1, b6 = R.ols_kept(X1, y, np.arange(p)), R.ols_kept(X6, y, np.arange(p))
        assert R.rel_err(b6[1:], b1[1:]) < 1e-8


@pytest.mark.parametrize("p,n", [(3, 9), (17, 18), (70, 145)])
def test_moment_kinds_describe_the_same_centered_moments(p, n):
    X, y = R.full_rank_design(p, n) if (p, n) in R.full_rank_cases() else \
        R._gauss_design(np.random.default_rng(p), n, p)
    Z = np.concatenate([X, y[:, None]], axis=1).astype(R.LD)
    mu = Z.sum(axis=0) / n
    C = (Z - mu).T @ (Z - mu)
    scale = np.sqrt(np.outer(np.diag(C), np.diag(C)))
    for kind in R.KINDS:
        G, s = R.moments(X, y, kind)
        assert G[0, 0] == n and s[0] == 0.0 and (G == G.T).all()
        if kind == "pooled":
            assert (G[0, 1:] == 0.0).all()
        if kind == "raw":
            assert (s == 0.0).all()
        if kind == "first":
            assert (s[1:] == np.r_[X[0], y[0]]).all()
        nn, m, Cg = R.centered_moments(G, s)
        assert nn == n
        # one rounding of a column sum whose terms are a few sd: far below 1e-14 sd
        assert float((np.abs(m - mu) / np.sqrt(np.diag(C) / n)).max()) < 1e-14
        # mean/sd < 1 here, so even the raw kind holds the centered moments to a few ulp
        assert float((np.abs(Cg - C) / scale).max()) < 1e-13, kind
    G, s = R.moments(np.zeros((0, p)), np.zeros(0), "first")
    assert not G.any() and not s.any()


@pytest.mark.parametrize("p", R.TOL_P)
def test_tol_pivot_is_clear_of_both_thresholds(p):
    X, y, j = R.tol_design(p)
    piv = R.scaled_pivots(X)
    assert 100 * R.TOL_KEEP <= piv[j] <= R.TOL_DROP / 100, float(piv[j])
    others = np.delete(piv, j)
    assert others.min() >= 100 * R.TOL_DROP, float(others.min())
    # with column j dropped the later pivots stay as clear
    piv2 = R.scaled_pivots(X, drop_below=R.TOL_DROP)
    assert np.delete(piv2, j).min() >= 100 * R.TOL_DROP


@pytest.mark.parametrize("p", R.DEFICIENT_P)
def test_deficient_designs_pivots(p):
    """Dependent columns have a (longdouble) pivot far below the default tol = 1e-10, every kept
    column one far above it."""
    for case in R.DEFICIENT_CASES:
        X, y, kept = R.deficient_design(p, case)
        piv = R.scaled_pivots(X, drop_below=1e-10)
        dropped = np.setdiff1d(np.arange(p), kept)
        assert (piv[dropped] < 1e-15).all(), case
        if len(kept):
            assert piv[kept].min() > 1e-4, case


def test_raw_constant_column_variance_is_noise_of_either_sign():
    """What the solver's drop rule sees for a constant column in raw moments: fp64 rounding noise.
    At least one design gives d > 0 (the former rule kept such a column), and (n + 3) 2^-53
    G[r][r] bounds every one of them while it is far below the d of every legitimate column."""
    positive = 0
    for p in R.DEFICIENT_P:
        for case in R.DEFICIENT_CASES:
            X, y, kept = R.deficient_design(p, case)
            if not case.startswith("const"):
                continue
            G, _ = R.moments(X, y, "raw")
            n = G[0, 0]
            for j in range(p):
                d = R.raw_variance_fp64(G, 1 + j)
                bound = (n + 3.0) * 2.0 ** -53 * G[1 + j, 1 + j]
                if j in kept:
                    assert d > 1e6 * bound
                else:
                    assert d <= bound
                    positive += d > 0
    assert positive > 0


def test_offset_raw_columns_stay_above_the_drop_bound():
    for p in R.OFFSET_P:
        X, y = R.offset_design(p, max(R.OFFSET_RATIOS))
        G, _ = R.moments(X, y, "raw")
        for j in range(p):
            d = R.raw_variance_fp64(G, 1 + j)
            assert d > 10 * (G[0, 0] + 3.0) * 2.0 ** -53 * G[1 + j, 1 + j]


def test_sequential_references():
    rng = np.random.default_rng(5)
    p, m = 19, 7
    b, x = rng.normal(size=p + 1), rng.normal(size=(p, m))
    s = R.predict_seq(b, x)
    for i in range(m):
        acc = b[0]
        for j in range(p):
            acc = acc + b[1 + j] * x[j, i]
        assert s[i] == acc
    ld, mag = R.predict_ld(b, x)
    assert float((np.abs(s - ld) / mag).max()) < 1e-13
    assert R.predict_seq(b[:1], x[:0])[0] == b[0]                    # p = 0
    mean, beta = rng.normal(size=p + 2), rng.normal(size=p + 1)
    Z = rng.normal(size=(p + 2, m))
    r = R.residual_seq(Z, p, p + 1, mean, beta)
    ref = (Z[p + 1] - mean[p + 1]) - (beta[1:] @ (Z[:p] - mean[1:p + 1, None]))
    assert np.abs(r - ref).max() < 1e-12
    assert abs(R.intercept_seq(p, mean, beta) - (mean[p + 1] - mean[1:p + 1] @ beta[1:])) < 1e-12


def test_fm_ref_edges():
    B = np.array([[1.0, 2.0], [np.nan, np.nan], [3.0, 2.0], [5.0, 2.0]])
    m, t = R.fm_ref(B, [1, 0, 2, 1])
    assert m.tolist() == [3.0, 2.0]
    assert t[0] == pytest.approx(3.0 / (2.0 / np.sqrt(3.0))) and t[1] == np.inf
    m, t = R.fm_ref(B, [0, 0, 0, 0])
    assert np.isnan(m).all() and np.isnan(t).all()
    m, t = R.fm_ref(B, [0, 0, 1, 0])
    assert m.tolist() == [3.0, 2.0] and np.isnan(t).all()
    m, t = R.fm_ref(-B, [1, 0, 1, 1])
    assert t[1] == -np.inf


def test_row_set_references():
    T, lda, A = 200, 64, 40
    v = R.presence(T, lda, A)
    assert not v[:, A:].any()
    assert not v[:, 0].any() and v[:, 1].sum() == 1 and v[:, 6].all()
    assert np.flatnonzero(v[:, 4]).tolist() == [63, 64]
    far = np.flatnonzero(v[:, 5])
    assert len(far) == 2 and far[0] < 64 and far[1] >= 192
    w = R.pack_words(v)
    for a in (1, 4, 5, 7, 15):
        for t in range(T):
            assert bool((int(w[t >> 6, a]) >> (t & 63)) & 1) == bool(v[t, a])
    # labels: pandas-style shift(-1) over the present days
    rng = np.random.default_rng(1)
    e, r = rng.normal(size=(T, lda)), rng.normal(size=(T, lda))
    sent = np.full((T, lda), -7.0)
    tg, tm = R.labels_ref(e, r, v, 0, T, sent, sent)
    days = np.flatnonzero(v[:, 7])
    assert (tg[days[:-1], 7] == e[days[1:], 7]).all() and np.isnan(tg[days[-1], 7])
    assert (tm[days[:-1], 7] == r[days[1:], 7]).all()
    assert (tg[~v] == -7.0).all()
    assert tg[days[-1:], 7].view(np.int64)[0] == R.NAN_BITS          # bitwise comparable on the GPU
    tg2, _ = R.labels_ref(e, r, v, 63, 65, sent, sent)
    inside = np.zeros_like(v)
    inside[63:65] = v[63:65]
    assert (tg2[~inside] == -7.0).all() and tg2[63, 4] == e[64, 4]
    # drop_last: only the last present day's bit goes, in its own word
    inw = rng.integers(0, 2 ** 64, size=w.shape, dtype=np.uint64)
    out = R.drop_last_ref(w, inw, np.zeros_like(w), 0, 4)
    diff = out ^ inw
    for a in range(lda):
        d = [int(t) for t in np.flatnonzero(v[:, a])]
        want = np.zeros(4, dtype=np.uint64)
        if d and (int(inw[d[-1] >> 6, a]) >> (d[-1] & 63)) & 1:
            want[d[-1] >> 6] = np.uint64(1 << (d[-1] & 63))
        assert (diff[:, a] == want).all()
    part = R.drop_last_ref(w, inw, np.full_like(w, 9), 1, 3)
    assert (part[[0, 3]] == 9).all() and (part[1:3] == out[1:3]).all()
    # row_bits: day by day
    ok = (rng.random(lda) < 0.8).astype(np.int32)
    for t0, t1 in [(0, 256), (65, 129), (63, 64), (130, 128), (70, 70), (1, 64)]:
        got = R.row_bits_ref(w, inw, ok, t0, t1)
        for c in range(4):
            m = sum(1 << s for s in range(64) if t0 <= 64 * c + s < t1)
            ref = (w[c] & inw[c] & np.uint64(m)) * ok.astype(np.uint64)
            assert (got[c] == ref).all()
