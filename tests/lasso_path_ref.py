"""Reference restatements for tests/test_lasso_path.py (test infrastructure, CPU only).

* ``oracle_chain``: scikit-learn's warm-started path (``lasso_path`` / ``LassoCV``) as a chain of
  the oracle's Gram coordinate descent, ``oracle_lasso_gram`` (oracle/lasso_oracle.c), with ``w``
  kept between alphas.  The oracle recomputes H = Q w from the start weights of every solve, as
  ``enet_coordinate_descent_gram`` does.
* ``lasso_cv_ref``: ``sklearn.LassoCV`` rebuilt from per-fold moments: the warm chain on each
  fold's train moments, the MSE of every model from the test fold's moments, the refit cold on
  the full-data moments.
"""
import ctypes

import numpy as np


def dense_design(n, p, seed):
    """The generator of tests/test_lasso.py::test_kernel_dense_fit_bit_exact_vs_oracle: correlated
    columns (6 common factors), ~40 % nonzero true coefficients, unit noise."""
    rng = np.random.default_rng(seed)
    F = rng.normal(size=(n, 6))
    X = F @ rng.normal(size=(6, p)) + 0.5 * rng.normal(size=(n, p))
    beta = np.where(rng.random(p) < 0.4, rng.normal(size=p), 0.0)
    y = X @ beta + rng.normal(size=n)
    return X, y


def raw_gram(X, y):
    """Raw moments [p+2][p+2] of [1, x, y] (afm's Gram layout with a zero shift)."""
    Z = np.concatenate([np.ones((len(y), 1)), X, y[:, None]], 1)
    return Z.T @ Z


def centered(X, y):
    """-> (n, Q, q, yy, x mean, y mean) of the centered design."""
    xm, ym = X.mean(0), y.mean()
    Xc, yc = X - xm, y - ym
    return len(y), Xc.T @ Xc, Xc.T @ yc, float(yc @ yc), xm, ym


def geom_alphas(alpha_max, n_alphas, eps=1e-3):
    return np.geomspace(alpha_max, alpha_max * eps, num=n_alphas)


def oracle_chain(Q, q, yy, alphas_n, *, max_iter=1000, tol=1e-4, positive=False, warm=True):
    """The oracle's descent at every l1 weight of ``alphas_n`` (alpha * n), in the order given,
    each solve started from the previous one's ``w`` (``warm``) or from zero ->
    (W [nalpha][p], info [nalpha][3] = {gap, tol * y'y, n_iter})."""
    import oracle
    L = oracle.lib()
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    p = len(q)
    w, H = np.zeros(p), np.zeros(p)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)          # noqa: E731
    W = np.empty((len(alphas_n), p))
    info = np.empty((len(alphas_n), 3))
    for i, an in enumerate(alphas_n):
        if not warm:
            w[:] = 0.0
        row = np.zeros(3)
        L.oracle_lasso_gram(p, P(Q), P(q), ctypes.c_double(float(yy)), ctypes.c_double(float(an)),
                            ctypes.c_double(0.0), int(max_iter), ctypes.c_double(float(tol)),
                            int(bool(positive)), P(w), P(H), P(row))
        W[i], info[i] = w, row
    return W, info


def kfold(n, k):
    """scikit-learn's unshuffled KFold."""
    sizes = np.full(k, n // k)
    sizes[:n % k] += 1
    idx, out, a = np.arange(n), [], 0
    for sz in sizes:
        out.append((np.concatenate([idx[:a], idx[a + sz:]]), idx[a:a + sz]))
        a += sz
    return out


def mse_from_moments(test, xm_tr, ym_tr, W):
    """MSE of the models (W [m][p], intercepts from the train means) on a dataset given by its
    centered moments ``test`` = (n, Q, q, yy, x mean, y mean)."""
    n, Q, q, yy, xm, ym = test
    out = np.empty(len(W))
    for i, w in enumerate(W):
        b0 = ym_tr - xm_tr @ w
        d = ym - b0 - xm @ w
        out[i] = (yy - 2 * (w @ q) + w @ Q @ w + n * d * d) / n
    return out


def lasso_cv_ref(X, y, n_alphas, folds, *, tol, max_iter, eps=1e-3):
    """-> dict(alphas, mse_path [n_alphas][n_folds], best, alpha, coef, intercept, n_iter)."""
    import oracle
    n, Q, q, yy, xm, ym = centered(X, y)
    alphas = geom_alphas(np.abs(q).max() / n, n_alphas, eps)
    mse = np.empty((len(folds), n_alphas))
    for k, (tr, te) in enumerate(folds):
        ntr, Qt, qt, yyt, xmt, ymt = centered(X[tr], y[tr])
        W, _ = oracle_chain(Qt, qt, yyt, alphas * ntr, max_iter=max_iter, tol=tol)
        mse[k] = mse_from_moments(centered(X[te], y[te]), xmt, ymt, W)
    best = int(np.argmin(np.mean(mse, axis=0)))
    w, gap, tol_y, it = oracle.lasso_gram(Q, q, yy, alphas[best] * n, max_iter=max_iter, tol=tol)
    return {"alphas": alphas, "mse_path": mse.T, "best": best, "alpha": alphas[best], "coef": w,
            "intercept": ym - xm @ w, "n_iter": it}
