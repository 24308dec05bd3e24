"""The mean-variance reference (tests/mv_ref.py) against its solver-independent KKT checker, on the
book grid the GPU tests use (no GPU needed).

Measured on this grid: every residual <= 6e-16, iterations <= 0.26 of the 4k + 8 cap."""
import numpy as np
import pytest

import mv_ref
from oracle import portfolio as P

KS = (2, 3, 11, 12, 32, 33, 64, 65, 100, 128)


def kind(b, w):
    nlo, nhi = int((w <= b["lo"] + 1e-14).sum()), int((w >= b["hi"] - 1e-14).sum())
    nfree = b["k"] - nlo - nhi
    if nfree == b["k"]:
        return "interior"
    if nfree == 0:
        return "vertex"
    return "both bounds beside free members" if nlo and nhi else "one bound"


@pytest.mark.parametrize("k", KS)
def test_reference_satisfies_kkt(k):
    worst, frac = 0.0, 0.0
    for b in mv_ref.book_grid(k):
        # rows >= 2k + 8: the pairwise covariance with holes stays positive definite
        assert b["rows"] >= 2 * k + 8 and np.linalg.eigvalsh(b["S"]).min() > 0
        for gamma, (w, it) in b["sol"].items():
            tag = (k, b["rows"], b["holes"], b["source"], gamma)
            assert abs(w.sum() - 1) < 1e-12, tag
            assert w.min() >= b["lo"] and w.max() <= b["hi"], tag
            res = mv_ref.kkt_residual(b["S"], b["mu"], gamma, w, b["lo"], b["hi"])
            worst, frac = max(worst, res), max(frac, it / (4 * k + 8))
            assert res < 1e-12, (tag, res)
            # a condition on the inputs: a capped device solve must not hide behind the reference
            assert 2 * it <= 4 * k + 8, (tag, it)
            # another: the reference's bound sets are unambiguous at the slack the GPU tests use
            assert not mv_ref.ambiguous_bounds(w, b["lo"], b["hi"]), tag
    print(f"k={k}: worst residual {worst:.2e}, worst iterations / cap {frac:.2f}")


@pytest.mark.parametrize("k", KS)
def test_gamma_zero_is_the_min_variance_solve(k):
    for b in mv_ref.book_grid(k):
        w, it = b["sol"][0.0]
        w0, it0 = P.box_qp_weights(b["S"], b["lo"], b["hi"])
        assert np.array_equal(w, w0) and it == it0, (k, b["rows"], b["holes"], b["source"])


def test_grid_has_every_kind_of_optimum():
    kinds = {kind(b, w) for k in KS for b in mv_ref.book_grid(k) for w, _ in b["sol"].values()}
    assert {"interior", "vertex", "both bounds beside free members"} <= kinds, kinds
    # the default cap at a large tolerance: ten names at hi, the rest at lo, none free
    assert any(int((w >= 0.1 - 1e-14).sum()) == 10 and int((w <= 1e-14).sum()) == 118
               for b in mv_ref.book_grid(128) for w, _ in b["sol"].values())


def test_vertex_rule_descends():
    """From a fully bound start that is not optimal, the release of (argmax g at hi, argmin g at
    lo) lowers the objective; the solve from the uniform start agrees with a brute-force search
    over the vertices when the return term dominates."""
    rng = np.random.default_rng(3)
    k, hi = 6, 0.5
    R = mv_ref.make_book(rng, k, 40, False)
    S, mu = P.pairwise_cov(R), rng.normal(0, 1e-3, k)
    gamma = 50.0
    w, _ = mv_ref.box_qp_mv(S, mu, gamma, 0.0, hi)
    best = min((0.5 * v @ S @ v - gamma * mu @ v, tuple(v))
               for i in range(k) for j in range(i + 1, k)
               for v in [np.where(np.isin(np.arange(k), (i, j)), hi, 0.0)])
    assert 0.5 * w @ S @ w - gamma * mu @ w <= best[0] + 1e-15
    assert mv_ref.kkt_residual(S, mu, gamma, w, 0.0, hi) < 1e-12
