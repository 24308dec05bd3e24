"""GPU parity of the mean-variance weight solve (afm_mean_variance_weights_f64: the wave solver for
books of up to 32 names, the workgroup solver above) against tests/mv_ref.py on the book grid of
tests/test_mv_ref.py: weights 1e-9 (the project's parity bar, tests/test_portfolio_gpu.py),
identical bound sets, the solver-independent KKT residual, and the covariance at the bars of the
existing weight tests."""
import numpy as np
import pytest

import mv_ref
from helpers import same

pytestmark = pytest.mark.gpu

# 32 | 33: wave solver -> workgroup solver; 64 | 65: the column-half and mask-word edge
KS = (2, 3, 12, 32, 33, 64, 65, 128)


def check_cov(cov, b):
    S, R = b["S"], b["R"]
    if b["k"] > 32:                                   # one-pass MFMA covariance
        assert np.abs(cov - S).max() <= 1e-12 * np.abs(S).max()
    elif np.isnan(R).any():
        assert same(cov, S)                           # nancorr(cov=True): bit-exact Welford
    else:
        assert np.abs(cov - S).max() <= 1e-13 * np.abs(S).max()


@pytest.mark.parametrize("k", KS)
def test_book_grid_vs_reference(k):
    from afm.portfolio import mean_variance_weights, min_variance_weights
    worst = 0.0
    for b in mv_ref.book_grid(k):
        lo, hi = b["lo"], b["hi"]
        mu_arg = None if b["source"] == "history" else b["mu"]
        w0, cov0 = min_variance_weights(b["R"], lo, hi)
        for gamma, (wo, it) in b["sol"].items():
            tag = (k, b["rows"], b["holes"], b["source"], gamma)
            w, cov, st = mean_variance_weights(b["R"], mu_arg, gamma, lo, hi, status=True)
            err = np.abs(w - wo).max()
            res = mv_ref.kkt_residual(b["S"], b["mu"], gamma, w, lo, hi)
            worst = max(worst, err)
            print(f"{tag}: |w - ref| {err:.2e} kkt {res:.2e} ref iterations {it}")
            assert st == 0, tag
            assert err < 1e-9, tag
            assert abs(w.sum() - 1) < 1e-12, tag
            assert np.array_equal(w <= lo + 1e-14, wo <= lo + 1e-14), tag
            assert np.array_equal(w >= hi - 1e-14, wo >= hi - 1e-14), tag
            assert res < 1e-9, tag
            check_cov(cov, b)
            if gamma == 0.0:
                assert same(w, w0) and same(cov, cov0), tag
    print(f"k={k}: worst |w - ref| {worst:.2e}")


def test_wide_cap_keeps_a_free_member():
    """hi = 0.15, k = 40: six names at hi leave 0.1 for a seventh, so no vertex is fully bound."""
    from afm.portfolio import mean_variance_weights
    from oracle import portfolio as P
    rng = np.random.default_rng([7, 40])
    R = mv_ref.make_book(rng, 40, 88, True)
    mu = rng.normal(0, 1e-3, 40)
    S = P.pairwise_cov(R)
    for gamma in (0.2, 5.0):
        wo, it = mv_ref.box_qp_mv(S, mu, gamma, 0.0, 0.15)
        assert 2 * it <= 4 * 40 + 8
        free = (wo > 1e-14) & (wo < 0.15 - 1e-14)
        assert free.any()
        w, cov, st = mean_variance_weights(R, mu, gamma, 0.0, 0.15, status=True)
        assert st == 0
        assert np.abs(w - wo).max() < 1e-9
        assert abs(w.sum() - 1) < 1e-12
        assert np.array_equal((w > 1e-14) & (w < 0.15 - 1e-14), free)
        assert mv_ref.kkt_residual(S, mu, gamma, w, 0.0, 0.15) < 1e-9


def test_single_feasible_point_and_non_finite_mu():
    """k * hi <= 1 keeps the shortcut (w = hi); a non-finite mu counts as 0."""
    from afm.portfolio import mean_variance_weights
    from oracle import portfolio as P
    rng = np.random.default_rng(5)
    R = mv_ref.make_book(rng, 10, 40, False)
    w, _ = mean_variance_weights(R, None, 1.0)
    assert same(w, np.full(10, 0.1))
    R = mv_ref.make_book(rng, 12, 40, False)
    mu = rng.normal(0, 1e-3, 12)
    mu[3], mu[7] = np.nan, np.inf
    wo, _ = mv_ref.box_qp_mv(P.pairwise_cov(R), mu, 0.2, 0.0, 0.2)
    w, _, st = mean_variance_weights(R, mu, 0.2, 0.0, 0.2, status=True)
    assert st == 0 and np.abs(w - wo).max() < 1e-9


@pytest.mark.parametrize("gamma", [-0.05, float("nan"), float("inf")])
def test_bad_gamma_is_rejected(gamma):
    from afm._lib import AfmError
    from afm.portfolio import mean_variance_weights
    R = mv_ref.make_book(np.random.default_rng(1), 12, 40, False)
    with pytest.raises(AfmError, match="gamma"):
        mean_variance_weights(R, None, gamma)
