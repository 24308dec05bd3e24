"""tests/xcorr_ref.py pinned on the CPU: the extended-precision per-pair correlation against
``DataFrame.corr()`` (identical NaN patterns, values within 1e-13; the 1e6-offset columns are left
out of that comparison -- pandas is the inaccurate side there -- and checked against an independent
per-pair statement instead), and the numpy statement of the summary."""
import functools

import numpy as np
import pandas as pd

import xcorr_ref as X


@functools.lru_cache(maxsize=None)
def inputs():
    return X.xcorr_inputs()


def pair_ref(x, y):
    """One pair, plainly: the jointly finite rows, two passes in np.longdouble."""
    ok = np.isfinite(x) & np.isfinite(y)
    if ok.sum() < 2:
        return np.nan
    a, b = x[ok].astype(np.longdouble), y[ok].astype(np.longdouble)
    da, db = a - a.sum() / len(a), b - b.sum() / len(b)
    va, vb = (da * da).sum(), (db * db).sum()
    if not (va > 0 and vb > 0):
        return np.nan
    return float(np.clip((da * db).sum() / np.sqrt(va * vb), -1, 1))


def test_kernel_constant_and_counts():
    c = X.kernel_constant("kXcRows")
    assert c % 4 == 0 and c >= 16
    counts = X.counts_all()
    assert set(X.COUNTS_X) | {c - 1, c, c + 1, 2 * c + 1} == set(counts)
    assert X.tolerance(600) == 32 * 600 * 2.0 ** -53 and X.tolerance(3) == X.tolerance(64)
    assert abs(X.tolerance(600) - 2.1e-12) < 0.05e-12


def test_inputs_have_every_kind_and_no_degenerate_pair():
    planes, rows_idx, nrows = inputs()
    assert planes.shape == (130, len(nrows), X.LDA)
    for t, n in enumerate(nrows):
        F = X.date_values(planes, rows_idx, nrows, t, np.arange(130))
        assert np.isfinite(F[:X.FINITE]).all()
        assert X.degenerate_pairs(F) == 0, int(n)
        assert X.spread(F) <= X.spread_max(n), (int(n), X.spread(F))
        if n >= 2:
            assert rows_idx[t, n - 1] == X.LDA - 1
            assert (F[X.CONST] == 0.75).all() and np.isfinite(F[X.ONEROW]).sum() == 1
            assert not (np.isfinite(F[X.EVEN]) & np.isfinite(F[X.ODD])).any()
            assert np.isinf(F[X.LAST][0]) and np.isnan(F[X.LAST][-1])
        if n >= 15:
            assert np.isnan(F[list(X.NAN5)]).any() and len(np.unique(F[X.TIES])) <= 7
        if n == X.ALLNAN_COUNT:
            assert np.isnan(F[X.ALLNAN]).all()
        if n >= 4:
            assert np.isinf(F[X.INFS]).any()
    assert np.isfinite(planes[:, :, :64]).mean() > 0.9       # the cells outside the rows: junk


def test_reference_matches_pandas_corr():
    planes, rows_idx, nrows = inputs()
    cols = np.array([p for p in range(130) if p not in (X.OFFSET, X.OFFNAN)])
    worst = 0.0
    for t, n in enumerate(nrows):
        F = X.date_values(planes, rows_idx, nrows, t, cols)
        ref = X.corr_ref(F)
        with np.errstate(all="ignore"):
            pdc = pd.DataFrame(F.T).replace([np.inf, -np.inf], np.nan).corr().to_numpy()
        if n == 0:
            assert np.isnan(ref).all()
            continue
        assert (np.isnan(ref) == np.isnan(pdc)).all(), int(n)
        if not np.isnan(ref).all():
            worst = max(worst, np.nanmax(np.abs(ref - pdc)))
        assert (ref == ref.T)[~np.isnan(ref)].all()
        d = np.diag(ref)
        assert ((d == 1.0) | np.isnan(d)).all()
    assert worst <= 1e-13, worst


def test_reference_rules_on_the_special_columns():
    planes, rows_idx, nrows = inputs()
    t = int(np.flatnonzero(nrows == X.ALLNAN_COUNT)[0])
    F = X.date_values(planes, rows_idx, nrows, t, np.arange(130))
    ref = X.corr_ref(F)
    for p in (X.CONST, X.CONSTNAN, X.ALLNAN, X.ONEROW):
        assert np.isnan(ref[p]).all() and np.isnan(ref[:, p]).all()
    assert np.isnan(ref[X.EVEN, X.ODD]) and ref[X.EVEN, X.EVEN] == 1.0
    for a, b, sign in X.COLLINEAR:
        assert abs(ref[a, b] - sign) < 1e-15 and abs(ref[a, b]) <= 1.0
    # the offset columns: against the plain per-pair statement (pandas loses 1e-11 there)
    for p in (X.OFFSET, X.OFFNAN):
        for q in (0, 1, X.NAN5[0], X.BIG, X.SMALL, X.INFS, X.OFFSET):
            want = pair_ref(F[p], F[q]) if p != q else 1.0
            assert abs(ref[p, q] - want) < 1e-17 or ref[p, q] == want, (p, q)
    assert abs(ref[X.BIG, X.SMALL] - pair_ref(F[X.BIG], F[X.SMALL])) < 1e-16


def test_reference_small_dates_pair_by_pair():
    planes, rows_idx, nrows = inputs()
    cols = [0, 1, X.TIES, X.CONST, X.OFFSET, 64, X.ONEROW, X.EVEN, X.ODD, X.INFS, X.LAST]
    for t, n in enumerate(nrows):
        if n > 17:
            continue
        F = X.date_values(planes, rows_idx, nrows, t, cols)
        ref = X.corr_ref(F)
        for i in range(len(cols)):
            for j in range(len(cols)):
                want = pair_ref(F[i], F[j])
                if i == j and not np.isnan(want):
                    want = 1.0
                assert (np.isnan(want) and np.isnan(ref[i, j])) or abs(ref[i, j] - want) < 1e-16


def test_z_inputs_keep_the_spread():
    planes, rows_idx, nrows = inputs()
    zs = X.zs_table()
    for cols, zc in ((X.Z_COLS, X.Z_COLS), (X.Z_IDENT, np.arange(len(X.Z_IDENT)))):
        for t, n in enumerate(nrows):
            F = X.date_values(planes, rows_idx, nrows, t, cols, zs, zc)
            assert X.degenerate_pairs(F) == 0, int(n)
            assert X.spread(F) <= X.spread_max(n), (int(n), X.spread(F))


def test_z_values_and_the_zero_row():
    planes, rows_idx, nrows = inputs()
    zs = X.zs_table(130)
    t = int(np.flatnonzero(nrows == 65)[0])
    F = X.date_values(planes, rows_idx, nrows, t, [3, 7, 9], zs)
    idx = rows_idx[t, :65]
    assert (F[0] == (planes[3, t, idx] - zs[3, idx, 0]) * zs[3, idx, 1]).all()
    assert (F[1] == 0).all()                                 # the {0, 0} row: constant
    assert np.isnan(X.corr_ref(F)[1]).all()


def test_summary_statement():
    """summary_ref against the statement of the issue, pair by pair: the count of non-NaN entries,
    np.where(isnan, 0, x).sum() of the pair's contiguous series over n; NaN for n == 0; a series
    longer than numpy's 8192-element reduction buffer."""
    rng = np.random.default_rng(5)
    nd, K = 9000, 3
    xc = rng.uniform(-1, 1, (nd, K, K))
    xc[rng.random(xc.shape) < 0.1] = np.nan
    xc[:, 0, 1] = np.nan
    xc[:, 2, 2] = np.nan
    xc[17, 2, 2] = -0.5
    st = X.summary_ref(xc)
    for j in range(K):
        for k in range(K):
            s = np.ascontiguousarray(xc[:, j, k])
            n = int((~np.isnan(s)).sum())
            assert st[j, k, 0] == n
            if n == 0:
                assert np.isnan(st[j, k, 1]) and np.isnan(st[j, k, 2])
            else:
                z = np.where(np.isnan(s), 0.0, s)
                assert st[j, k, 1] == z.sum() / n and st[j, k, 2] == np.abs(z).sum() / n
    assert st[0, 1, 0] == 0 and st[2, 2, 0] == 1 and st[2, 2, 1] == -0.5 and st[2, 2, 2] == 0.5
    assert abs(st[1, 1, 1] - np.nanmean(xc[:, 1, 1])) < 1e-14
