"""tests/gbt_shap_ref.py against itself (no GPU): the pinned per-path statement of
include/afm_gbt_shap.h against the Shapley values by definition (every subset, np.longdouble)
within the derived bound of the module's docstring, the efficiency identity against
gbt_ref.predict, a never-split column, the cover against a fit's own sums, and an exact grid on
which the pinned statement and the definition agree bit for bit."""
import numpy as np
import pytest

import gbt_ref as R
import gbt_shap_ref as S


def _cells(rng, Xc, n):
    """Cells to explain: rows of the covering sample and fresh ones, some exactly on a threshold."""
    X = np.round(rng.standard_normal((n, Xc.shape[1])) * 4) / 4
    X[: n // 2] = Xc[rng.integers(0, len(Xc), size=n // 2)]
    return X


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6])
def test_pinned_against_the_definition_within_the_bound(D):
    rng = np.random.default_rng(100 + D)
    p, n_trees = 9, 12
    feat, thr, val, cov, Xc = S.random_trees(rng, n_trees, D, p)
    assert (feat >= 0).sum() >= n_trees and (cov[feat != S.ABSENT] >= 1).all()
    X = _cells(rng, Xc, 96)
    assert any((X[:, feat[r, 0]] == thr[r, 0]).any() for r in range(n_trees))   # on a threshold
    for R_ in (n_trees, 5):
        got = S.contribs_pinned(X, feat, thr, val, cov, 0.125, R_)
        want = S.contribs_by_definition(X, feat, thr, val, cov, 0.125, R_)
        E = S.bound(feat, val, 0.125, R_)
        err = np.abs(got.astype(np.longdouble) - want).max()
        print(f"D={D} trees={R_}: max error {float(err):.3e} = {float(err / E):.4f} E")
        assert err <= 2 * E
        # efficiency: the row sums are the prediction (exactly for the definition, up to
        # the columns' errors and the walk's own additions for the pinned statement)
        pred = R.predict(X, feat, thr, val, 0.125, R_)
        assert np.abs(want.sum(axis=1) - pred).max() <= E
        assert np.abs(got.astype(np.longdouble).sum(axis=1) - pred).max() <= (p + 1) * 2 * E + E
        # a column no tree splits on is +0.0 exactly
        unused = sorted(set(range(p)) - set(feat[:R_][feat[:R_] >= 0].tolist()))
        assert unused
        assert (got[:, unused] == 0).all() and not np.signbit(got[:, unused]).any()


def test_root_leaf_no_tree_and_one_column_chain():
    X = np.array([[0.5, -1.0], [2.0, 3.0]])
    feat = np.array([[S.LEAF, S.ABSENT, S.ABSENT]], np.int32)
    val = np.array([[0.375, 0.0, 0.0]])
    cov = np.array([[10, 0, 0]], np.int64)
    got = S.contribs_pinned(X, feat, np.zeros((1, 3)), val, cov, 0.25)
    assert got.tolist() == [[0.0, 0.0, 0.625]] * 2
    assert S.contribs_pinned(X, feat, np.zeros((1, 3)), val, cov, 0.25, 0).tolist() == \
        [[0.0, 0.0, 0.25]] * 2
    # one column split twice: m = 1, z = the product of both ratios, s = 1
    feat = np.array([[1, 1, S.LEAF, S.LEAF, S.LEAF, S.ABSENT, S.ABSENT]], np.int32)
    thr = np.array([[1.0, 0.0, 0, 0, 0, 0, 0]])
    val = np.array([[0.0, 0.0, 3.0, 1.0, 2.0, 0, 0]])
    cov = np.array([[12, 9, 3, 6, 3, 0, 0]], np.int64)
    got = S.contribs_pinned(X, feat, thr, val, cov)
    want = S.contribs_by_definition(X, feat, thr, val, cov)
    assert np.abs(got - want).max() <= 2 * S.bound(feat, val)
    mean = (3 * 3.0 + 6 * 1.0 + 3 * 2.0) / 12
    assert np.allclose(got[:, 2], mean) and np.allclose(got[:, 1], [1.0 - mean, 3.0 - mean])
    assert (got[:, 0] == 0).all()


def test_cover_is_the_fits_own_sums():
    rng = np.random.default_rng(3)
    n, p = 500, 4
    X = np.round(rng.standard_normal((n, p)) * 8) / 8
    y = 0.05 * (X[:, 1] > 0.25) - 0.03 * (X[:, 2] < -0.5) + 0.01 * rng.standard_normal(n)
    w = rng.integers(0, 3, size=n).astype(np.int32)
    fit = R.fit(X, y, w, n_rounds=5, max_depth=3, eta=0.3, max_bin=32)
    cov = S.cover(fit["bins"], w, fit["feat"], fit["bin"])
    assert (cov[:, 0] == w.sum()).all()
    r, v = np.nonzero(fit["feat"] >= 0)
    assert len(r) > 10 and (cov[r, v] == cov[r, 2 * v + 1] + cov[r, 2 * v + 2]).all()
    assert (cov[fit["feat"] == S.ABSENT] == 0).all() and (cov[fit["feat"] != S.ABSENT] >= 1).all()
    # the raw-value walk partitions the rows like the bins: the leaves' covers from predict's rule
    for r in range(5):
        for v in np.flatnonzero(fit["feat"][r] == S.LEAF):
            at = np.ones(n, dtype=bool)
            c = v
            while c:
                a = (c - 1) // 2
                at &= (X[:, fit["feat"][r, a]] < fit["thr"][r, a]) == (c == 2 * a + 1)
                c = a
            assert cov[r, v] == w[at].sum()


def _grid_trees():
    """Every shape of depth <= 2 with halving covers and leaf values in eighths; at most two
    columns a tree, so that the enumeration's own weights (over the columns the tree uses) are in
    {1, 1/2} like the paths'."""
    L, A = S.LEAF, S.ABSENT
    shapes = [[0, L, L, A, A, A, A], [0, 1, L, L, L, A, A], [1, L, 0, A, A, L, L],
              [0, 1, 1, L, L, L, L], [0, 0, 1, L, L, L, L], [2, 2, 2, L, L, L, L]]
    feat = np.array(shapes, np.int32)
    cov = np.zeros(feat.shape, np.int64)
    cov[:, 0] = 64
    for v in range(1, 7):
        cov[:, v] = np.where(feat[:, v] != A, cov[:, (v - 1) // 2] // 2, 0)
    rng = np.random.default_rng(4)
    thr = np.where(feat >= 0, rng.integers(-4, 5, size=feat.shape) / 4, 0.0)
    val = np.where(feat == L, rng.integers(-16, 17, size=feat.shape) / 8, 0.0)
    return feat, thr, val, cov


def test_exact_grid_pinned_equals_the_definition_bit_for_bit():
    """D <= 2, power-of-two covers, values in eighths: z in {1/2, 1/4}, m <= 2, W in {1, 1/2} --
    every operation is exact, so the fp64 statement equals the longdouble enumeration."""
    feat, thr, val, cov = _grid_trees()
    rng = np.random.default_rng(5)
    X = rng.integers(-6, 7, size=(64, 3)) / 4
    got = S.contribs_pinned(X, feat, thr, val, cov, 0.5)
    want = S.contribs_by_definition(X, feat, thr, val, cov, 0.5)
    assert (got.astype(np.longdouble) == want).all()
    assert got.tobytes() == want.astype(np.float64).tobytes()
    assert (got.sum(axis=1) == R.predict(X, feat, thr, val, 0.5)).all()
    assert np.abs(got[:, :3]).max() > 0.5


def test_agg_pinned_is_the_sum_and_the_count():
    rng = np.random.default_rng(6)
    c = rng.standard_normal((3, 5, 128))
    use = rng.random((3, 128)) < 0.7
    use[1] = False
    c[~np.broadcast_to(use[:, None, :], c.shape)] = np.nan
    agg, cnt = S.agg_pinned(c, use)
    assert cnt.tolist() == use.sum(axis=1).tolist() and (agg[1] == 0).all()
    x = np.where(use[:, None, :], c, 0.0)
    assert np.allclose(agg[..., 0], x.sum(axis=2)) and np.allclose(agg[..., 1], np.abs(x).sum(axis=2))
