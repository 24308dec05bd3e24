"""tests/gbt_ref.py -- the numpy statement of the boosted-tree algorithm (include/afm_gbt.h) --
against exact arithmetic, against itself (binned fit == raw tree walk) and against scikit-learn.
No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

import gbt_ref as R


def test_histogram_sums_equal_python_int_sums():
    rng = np.random.default_rng(0)
    n, p, B, nnodes = 500, 3, 16, 4
    bins = rng.integers(0, B, size=(p, 512)).astype(np.uint8)
    node = rng.integers(-1, nnodes, size=n).astype(np.int32)
    w = rng.integers(0, 3, size=n).astype(np.int32)
    q = (rng.integers(-2 ** 52, 2 ** 52, size=n) * w).astype(np.int64)
    h = R.histogram(bins, node, q, w, nnodes, B)
    want = {}
    for i in range(n):
        if node[i] < 0:
            continue
        for k in range(p):
            key = (int(node[i]), k, int(bins[k, i]))
            a, b = want.get(key, (0, 0))
            want[key] = (a + int(q[i]), b + int(w[i]))
    for j in range(nnodes):
        for k in range(p):
            for b in range(B):
                assert (int(h[j, k, b, 0]), int(h[j, k, b, 1])) == want.get((j, k, b), (0, 0))


def test_stump_on_dyadic_inputs_equals_an_exhaustive_fraction_search():
    rng = np.random.default_rng(1)
    n, p = 40, 3
    X = rng.integers(-8, 8, size=(n, p)) / 4.0
    y = rng.integers(-64, 64, size=n) / 128.0
    w = np.ones(n, dtype=np.int32)
    r = R.fit(X, y, w, n_rounds=1, max_depth=1, eta=1.0, reg_lambda=0.0, max_bin=256)
    # exhaustive: every (column, distinct value c) with "x < c goes left", gain in exact rationals
    g = [Fraction(-float(v)) for v in y]                    # F = 0: g = -y
    G, best = sum(g), None
    for k in range(p):
        for c in sorted(set(X[:, k])):
            L = [g[i] for i in range(n) if X[i, k] < c]
            if not L or len(L) == n:
                continue
            GL = sum(L)
            gain = GL * GL / len(L) + (G - GL) ** 2 / (n - len(L)) - G * G / n
            if best is None or gain > best[0]:
                best = (gain, k, float(c), GL, len(L))
    gain, k, c, GL, HL = best
    assert gain > 0
    assert (r["feat"][0, 0], r["thr"][0, 0]) == (k, c)
    assert r["val"][0, 1] == float(-GL / HL) and r["val"][0, 2] == float(-(G - GL) / (n - HL))
    assert r["val"][0, 0] == float(-G / n)
    assert list(r["feat"][0, 1:]) == [R.LEAF, R.LEAF]


def _walk_case(seed, B=16):
    rng = np.random.default_rng(seed)
    n, p = 600, 6
    X = rng.standard_normal((n, p))
    X[:, 3] = X[:, 1]                                       # a duplicated column
    X[:, 4] = np.round(X[:, 4])                             # heavy ties: fewer than B - 1 cuts
    y = 0.05 * (X[:, 1] > 0.3) + 0.02 * X[:, 0] * X[:, 2] + 0.01 * rng.standard_normal(n)
    w = rng.integers(0, 3, size=n).astype(np.int32)
    return X, y, w, B


@pytest.mark.parametrize("seed", [0, 1])
def test_tree_walk_over_raw_values_is_bit_equal_to_the_binned_fit(seed):
    X, y, w, B = _walk_case(seed)
    r = R.fit(X, y, w, n_rounds=12, max_depth=3, eta=0.3, reg_lambda=1.0, max_bin=B,
              base_score=0.01)
    assert (w == 0).any() and (w == 2).any()
    got = R.predict(X, r["feat"], r["thr"], r["val"], base_score=0.01)
    assert np.array_equal(got, r["F"])
    split = r["feat"][r["feat"] >= 0]
    assert len(split) > 20 and (split == 1).any()
    assert not (split == 3).any()                           # never the copy over the first
    assert r["ncuts"][4] < B - 1 and (r["ncuts"][[0, 1, 2]] == B - 1).all()


def test_moments_and_metrics():
    rng = np.random.default_rng(3)
    F, y = rng.standard_normal(50), rng.standard_normal(50)
    w = (np.arange(50) % 3).astype(np.int32)
    ev = R.moments(F, y, w)
    assert ev[0, 0] + ev[1, 0] == 50 and ev[1, 0] == 17
    rmse, ic = R.metrics(ev[0])
    m = w > 0
    assert abs(rmse - np.sqrt(np.mean((F[m] - y[m]) ** 2))) < 1e-14
    assert abs(ic - np.corrcoef(F[m], y[m])[0, 1]) < 1e-13


SKLEARN_BOUND = 16 * 3.47e-18


def test_cross_check_against_scikit_learn():
    """With a bin for every distinct value, lambda = 0, depth 3 and 20 rounds the training
    predictions are those of scikit-learn's GradientBoostingRegressor(criterion='squared_error',
    init='zero') up to summation order.  Measured with scikit-learn 1.7.2 / numpy 2.2.6 (n = 200,
    p = 5, |y| <= 0.064): the largest difference over seeds 0-4 is 3.47e-18 (per seed 3.47e-18,
    3.47e-18, 1.73e-18, 3.47e-18, 3.47e-18: one or two units in the last place of a prediction near
    0.01); the bound is 16 times that, the room for another summation order in numpy's means."""
    from sklearn import ensemble
    worst = 0.0
    for seed in range(5):
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((200, 5))
        y = 0.02 * np.tanh(X[:, 0] * X[:, 1] + X[:, 2])
        assert np.abs(y).max() <= 0.064
        r = R.fit(X, y, np.ones(200, np.int32), n_rounds=20, max_depth=3, eta=0.1,
                  reg_lambda=0.0, max_bin=256)
        assert (r["ncuts"] >= 199).all()                  # a cut at every distinct value
        m = ensemble.GradientBoostingRegressor(
            criterion="squared_error", init="zero", n_estimators=20, max_depth=3,
            learning_rate=0.1, random_state=0).fit(X, y)
        d = float(np.abs(m.predict(X) - r["F"]).max())
        print(f"seed {seed}: max |ref - sklearn| = {d:.3e}")
        worst = max(worst, d)
    assert worst <= SKLEARN_BOUND
