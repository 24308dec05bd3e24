"""tests/risk_ref.py against closed forms and against itself (no GPU): West's update and the
specific-variance recurrence against the weighted sums in longdouble, lambda = 1 against np.cov,
symmetry in bits, positive semi-definiteness of S, the unused-date / min_obs / lag boundaries, the
net book, and the summation order of the fill against numpy."""
import numpy as np
import pytest

import risk_ref as R
from helpers import same

U = 2.0 ** -53


def case(T=60, K1=4, seed=0):
    rng = np.random.default_rng(seed)
    vol = rng.uniform(0.002, 0.02, K1)
    L = np.linalg.cholesky(0.5 * np.eye(K1) + 0.5)
    beta = (rng.standard_normal((T, K1)) @ L.T) * vol + rng.normal(0, 1e-3, K1)
    return beta, np.full(T, K1 - 1, dtype=np.int32)


@pytest.mark.parametrize("T,K1,hl", [(60, 4, 20.0), (200, 8, 90.0), (40, 32, 5.0)])
def test_west_update_against_the_weighted_sums(T, K1, hl):
    """The recurrence differs from the closed form (longdouble) by no more than 64 times what the
    recurrence itself moves between fp64 and longdouble on the same case."""
    beta, rank = case(T, K1, seed=T)
    f64, n = R.factor_cov(beta, rank, hl, 1, 0)
    fld, _ = R.factor_cov(beta, rank, hl, 1, 0, dtype=R.LD)
    assert n.tolist() == list(range(1, T + 1))
    for t in (1, T // 2, T - 1):
        closed = R.factor_cov_closed(beta[:t + 1], hl)
        scale = float(np.abs(closed).max())
        own = float(np.abs(f64[t].astype(R.LD) - fld[t]).max()) / scale
        diff = float(np.abs(f64[t].astype(R.LD) - closed).max()) / scale
        print(f"T={T} K1={K1} t={t}: closed-form diff {diff:.2e}, own fp64-longdouble {own:.2e}, "
              f"ratio {diff / own if own else float('nan'):.2f}")
        assert own > 0 and diff <= 64 * own
        assert float(np.abs(fld[t] - closed).max()) / scale < 1e-17


def test_specific_recurrence_against_the_weighted_sum():
    rng = np.random.default_rng(3)
    u = rng.normal(0, 0.02, (80, 5))
    u[rng.random((80, 5)) < 0.2] = np.nan
    s64, _ = R.specific(u, 30.0, 1, 0)
    sld, _ = R.specific(u, 30.0, 1, 0, dtype=R.LD)
    for a in range(5):
        closed = R.specific_closed(u[:, a], 30.0)
        own = abs(R.LD(s64[-1, a]) - sld[-1, a]) / closed
        diff = abs(R.LD(s64[-1, a]) - closed) / closed
        print(f"security {a}: diff {float(diff):.2e} own {float(own):.2e}")
        assert own > 0 and diff <= 64 * own


def test_lambda_one_is_the_population_covariance():
    """An infinite half-life weighs every date alike: np.cov(ddof=0), to rounding."""
    beta, rank = case(50, 5, seed=9)
    f, _ = R.factor_cov(beta, rank, np.inf, 1, 0)
    assert R.decay(np.inf) == 1.0
    ref = np.cov(beta.T, ddof=0)
    assert np.abs(f[-1] - ref).max() <= 64 * 50 * U * np.abs(ref).max()
    u = np.random.default_rng(2).normal(0, 0.01, (40, 3))
    s, _ = R.specific(u, np.inf, 1, 0)
    assert np.allclose(s[-1], (u * u).mean(axis=0), rtol=1e-13, atol=0)


def test_fcov_and_book_covariance_are_symmetric_in_bits_and_psd():
    rng = np.random.default_rng(11)
    T, p, A = 70, 6, 40
    beta, rank = case(T, p + 1, seed=5)
    f, _ = R.factor_cov(beta, rank, 15.0, 5, 1)
    for t in range(T):
        assert same(f[t], f[t].T)
    X = rng.standard_normal((p, T, A))
    X[:, :, 3] = np.nan
    spec = rng.uniform(1e-5, 1e-3, (T, A))
    for k in (1, 2, 10, 33):
        mem = rng.choice(A, size=k, replace=False)
        w = rng.dirichlet(np.ones(k))
        r = R.book(X, T - 1, mem, w, f[T - 1], spec[T - 1], 1e-4)
        S = r["S"]
        assert r["status"] == 0 and same(S, S.T)
        ev = np.linalg.eigvalsh(S)
        assert ev.min() >= -64 * U * np.trace(S)
        # the risk numbers are the quadratic form of S to rounding, and add up exactly
        tot, fv, sv, filled = r["risk"]
        assert tot == fv + sv and filled == 0
        assert abs(w @ S @ w - tot) <= 64 * (p + 1 + k) * U * tot
        terms = np.abs(r["contrib"]).sum()
        assert abs(r["contrib"].sum() - fv) <= (p + 1) * U * terms
    # without the specific term S = B F B' is singular for k > K1 and still not indefinite
    r = R.book(X, T - 1, np.arange(20), np.full(20, 0.05), f[T - 1], np.zeros(A), 0.0)
    assert np.linalg.eigvalsh(r["S"]).min() >= -64 * U * np.trace(r["S"])


def test_unused_dates_min_obs_and_lag():
    beta, rank = case(30, 3, seed=1)
    rank = rank.copy()
    rank[[4, 9]] = 1                                  # a dropped regressor
    beta[[6, 7]] = np.nan                             # too few rows: no coefficients
    beta[12, 1] = np.inf
    used = R.used_dates(beta, rank)
    assert np.flatnonzero(~used).tolist() == [4, 6, 7, 9, 12]
    keep = np.flatnonzero(used)
    f0, n0 = R.factor_cov(beta, rank, 10.0, 1, 0)
    fc, nc = R.factor_cov(beta[keep], rank[keep], 10.0, 1, 0)
    for j, t in enumerate(keep):                      # an unused date updates nothing
        assert same(f0[t], fc[j]) and n0[t] == nc[j] == j + 1
    for t in np.flatnonzero(~used):
        assert same(f0[t], f0[t - 1]) and n0[t] == n0[t - 1]
    for lag in (0, 1, 3):
        for min_obs in (1, 5, 25, 26):
            f, n = R.factor_cov(beta, rank, 10.0, min_obs, lag)
            assert n[:lag].tolist() == [0] * lag and same(n[lag:], n0[:30 - lag])
            for t in range(30):
                if t < lag or n0[t - lag] < min_obs:
                    assert np.isnan(f[t]).all()
                else:
                    assert same(f[t], f0[t - lag])
    assert int(n0[-1]) == 25                          # min_obs 25: the last date only; 26: never
    assert np.isfinite(R.factor_cov(beta, rank, 10.0, 25, 0)[0][-1]).all()
    assert np.isnan(R.factor_cov(beta, rank, 10.0, 26, 0)[0]).all()
    # the specific variance counts a security's own observations
    u = np.random.default_rng(0).normal(0, 0.01, (30, 4))
    u[:, 0] = np.nan                                  # never present
    u[:12, 1] = np.nan                                # listed late
    u[20:, 2] = np.nan                                # stops: its state is carried
    s, fill = R.specific(u, 10.0, 5, 1)
    assert np.isnan(s[:, 0]).all()
    assert np.isnan(s[:17, 1]).all() and np.isfinite(s[17:, 1]).all()
    assert same(s[21:, 2], np.repeat(s[21, 2], 9)) and np.isfinite(s[5:, 3]).all()
    assert np.isnan(s[:5]).all() and np.isnan(fill[:5]).all()
    assert fill[10] == s[10, 2:].sum() / 2.0 and fill[25] == s[25, 1:].sum() / 3.0


def test_residuals_mask_everything_that_is_not_a_used_finite_row():
    rng = np.random.default_rng(6)
    p, T, A = 3, 8, 10
    X = rng.standard_normal((p, T, A))
    y = rng.standard_normal((T, A))
    beta = rng.standard_normal((T, p + 1))
    rank = np.full(T, p, dtype=np.int32)
    rank[2] = p - 1
    beta[5, 0] = np.nan
    mask = rng.random((T, A)) < 0.8
    X[1, 3, 4], y[4, 7] = np.nan, np.inf
    u = R.residuals(X, y, mask, beta, rank)
    assert np.isnan(u[2]).all() and np.isnan(u[5]).all()
    assert np.isnan(u[3, 4]) and np.isnan(u[4, 7]) and np.isnan(u[~mask]).all()
    t, a = 0, int(np.flatnonzero(mask[0])[0])
    acc = beta[t, 0]
    for j in range(p):
        acc = acc + beta[t, j + 1] * X[j, t, a]
    assert u[t, a] == y[t, a] - acc
    ok = mask & np.isfinite(u)
    assert ok.sum() == (mask[[0, 1, 3, 4, 6, 7]]).sum() - mask[3, 4] - mask[4, 7]


def test_net_book_counts_a_name_on_both_sides_once():
    mem, h = R.net_book([5, 2, 9], np.array([0.5, 0.3, 0.2]), [7, 2, 1], np.array([0.6, 0.3, 0.1]))
    assert mem.tolist() == [5, 2, 9, 7, 1]
    assert h.tolist() == [0.25, 0.0, 0.1, -0.3, -0.05]
    rng = np.random.default_rng(8)
    p, T, A = 2, 3, 12
    X = rng.standard_normal((p, T, A))
    beta, rank = case(T, p + 1, seed=2)
    F = R.factor_cov(beta, rank, 5.0, 1, 0)[0][-1]
    spec = rng.uniform(1e-4, 1e-3, (T, A))
    spec[2, 7] = np.nan                               # filled from the date's mean
    r = R.book(X, 2, mem, h, F, spec[2], 5e-4, cov=False)
    assert r["status"] == 0 and r["S"] is None and r["risk"][3] == 1
    # the same holdings as a dense vector
    hv = np.zeros(A)
    hv[mem] = h
    B = np.c_[np.ones(A), X[:, 2].T]
    d = np.where(np.isfinite(spec[2]), spec[2], 5e-4)
    tot = hv @ (B @ F @ B.T + np.diag(d)) @ hv
    assert abs(r["risk"][0] - tot) <= 1e-13 * tot
    # no fill to give: the date is flagged
    bad = R.book(X, 2, mem, h, F, spec[2], np.nan, cov=False)
    assert bad["status"] == 4 and np.isnan(bad["risk"]).all() and np.isnan(bad["contrib"]).all()
    nof = R.book(X, 2, mem, h, np.full_like(F, np.nan), spec[2], 5e-4)
    assert nof["status"] == 4 and np.isnan(nof["S"]).all()


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 127, 128, 129, 1000, 8191, 8192, 8193, 10000, 20000])
def test_fill_summation_order_is_numpys(n):
    v = np.random.default_rng(n).uniform(1e-5, 1e-3, n)
    assert R.np_sum_stated(v) == R.np_sum(v)
