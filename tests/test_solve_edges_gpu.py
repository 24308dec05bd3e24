"""afm_ols_solve_f64 at the shapes chosen to break it: tile and register boundaries of p, n = p + 1,
under-determined segments mixed into one launch, rank-deficient designs, the tol argument and
column offsets, in the three moment representations the solver meets (tests/ols_ref.py).

Moments are built on the host in longdouble and copied to the device, so the input is deterministic
and independent of the Gram kernels.  Accuracy bar: the project's max |b - ref| / max |ref| < 1e-9
(tests/test_regression_gpu.py, BASELINE) against longdouble least squares.  Every design asserted
at it has cond_scaled <= 300 (tests/test_ols_ref.py), so cond^2 * 2^-53 * 10 <= 1e-10.  Because the
column scales spread over 1e-6 .. 1e6, the same bar is also applied to the slopes in units of their
column's standard deviation, where no large coefficient hides the others.

Raw moments (shift = 0) lose (mean / sd)^2 * eps on a kept column: asserted at 1e-9 only up to
mean / sd = 1e2; the measured figures at 1e4 and 1e6 are recorded in DESIGN.md.
"""
import functools

import numpy as np
import pytest

import ols_ref as R

pytestmark = pytest.mark.gpu

BAR = 1e-9


def _solve(moms, p, tol=1e-10):
    """[(gram, shift)] -> (beta [nseg][p+1], nobs [nseg], rank [nseg]) from one launch."""
    import torch
    from afm.regression import ols_solve
    G = torch.from_numpy(np.stack([m[0] for m in moms])).cuda()
    S = torch.from_numpy(np.stack([m[1] for m in moms])).cuda()
    beta, nobs, rank = ols_solve(G, S, p, tol)
    torch.cuda.synchronize()
    return beta.cpu().numpy(), nobs.cpu().numpy(), rank.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _full(p, n):
    X, y = R.full_rank_design(p, n)
    return X, y, R.ols_kept(X, y, np.arange(p))


@functools.lru_cache(maxsize=None)
def _under(p, k):
    X, y = R.under_determined_design(p, k)
    return X, y, (R.ols_kept(X, y, np.arange(p)) if len(y) > p else None)


@functools.lru_cache(maxsize=None)
def _deficient(p, case):
    X, y, kept = R.deficient_design(p, case)
    return X, y, kept, R.ols_kept(X, y, kept)


@functools.lru_cache(maxsize=None)
def _tol(p):
    X, y, j = R.tol_design(p)
    kept = np.array([c for c in range(p) if c != j])
    return X, y, j, R.ols_kept(X, y, kept)


@functools.lru_cache(maxsize=None)
def _offset(p, ratio):
    X, y = R.offset_design(p, ratio)
    return X, y, R.ols_kept(X, y, np.arange(p))


def _errors(beta, ref, X, kept):
    """(the project's figure on [intercept, slopes], the same on the kept slopes in sd units)."""
    e = R.rel_err(beta, ref)
    if len(kept) == 0:
        return e, 0.0
    sd = X[:, kept].std(axis=0)
    return e, R.rel_err(beta[1 + kept] * sd, ref[1 + kept] * sd)


def _check(beta, ref, X, kept, what):
    e, es = _errors(beta, ref, X, kept)
    print(f"{what}: rel err {e:.3e}, slopes in sd units {es:.3e}")
    assert e < BAR and es < BAR, what


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("p,n", R.full_rank_cases())
def test_full_rank(p, n, kind):
    X, y, ref = _full(p, n)
    beta, nobs, rank = _solve([R.moments(X, y, kind)], p)
    assert nobs[0] == n and rank[0] == p
    _check(beta[0], ref, X, np.arange(p), f"full p={p} n={n} {kind}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("p", R.UNDER_P)
def test_under_determined_segments_in_one_launch(p, kind):
    ns = R.under_determined_ns(p)
    assert sorted(set(ns)) == sorted({0, 1, p - 1, p, p + 1, 2 * p + 5}) and len(ns) == 9
    data = [_under(p, k) for k in range(9)]
    moms = [R.moments(X, y, kind) for X, y, _ in data]
    beta, nobs, rank = _solve(moms, p)
    assert nobs.tolist() == ns
    for k, n in enumerate(ns):
        if n <= p:
            assert np.isnan(beta[k]).all() and rank[k] == 0, (k, n)
            continue
        alone, nobs1, rank1 = _solve([moms[k]], p)
        assert (beta[k].view(np.int64) == alone[0].view(np.int64)).all(), (k, n)
        assert rank[k] == rank1[0] == p and nobs1[0] == n
        _check(beta[k], data[k][2], data[k][0], np.arange(p), f"under p={p} seg={k} n={n} {kind}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", R.DEFICIENT_CASES)
@pytest.mark.parametrize("p", R.DEFICIENT_P)
def test_rank_deficient(p, case, kind):
    """The dependent column (a later duplicate, a combination of earlier columns, a constant) is
    dropped with coefficient exactly 0.0 and the rest is the regression on the kept columns.  A
    constant column in raw moments has rounding noise for a variance: it is dropped because it has
    no resolvable variance (include/afm.h), where a d > 0 rule kept it when the noise was
    positive."""
    X, y, kept, ref = _deficient(p, case)
    beta, nobs, rank = _solve([R.moments(X, y, kind)], p)
    dropped = np.setdiff1d(np.arange(p), kept)
    print(f"deficient p={p} {case} {kind}: rank {rank[0]} (expected {len(kept)}), dropped "
          f"coefficients {beta[0][1 + dropped][:4]}")
    assert nobs[0] == len(y)
    assert rank[0] == len(kept)
    assert (beta[0][1 + dropped] == 0.0).all()
    _check(beta[0], ref, X, kept, f"deficient p={p} {case} {kind}")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("p", R.TOL_P)
def test_tol_keeps_or_drops_a_near_duplicate(p, kind):
    """Column j = an earlier column + delta * noise with a scaled pivot 100x clear of both
    thresholds (tests/test_ols_ref.py): kept at tol = 1e-10, dropped at tol = 1e-4."""
    X, y, j, ref_dropped = _tol(p)
    mom = R.moments(X, y, kind)
    beta, _, rank = _solve([mom], p, R.TOL_KEEP)
    assert rank[0] == p and beta[0][1 + j] != 0.0
    beta, _, rank = _solve([mom], p, R.TOL_DROP)
    assert rank[0] == p - 1 and beta[0][1 + j] == 0.0
    kept = np.array([c for c in range(p) if c != j])
    _check(beta[0], ref_dropped, X, kept, f"tol p={p} {kind} dropped")


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("ratio", R.OFFSET_RATIOS)
@pytest.mark.parametrize("p", R.OFFSET_P)
def test_column_offsets(p, ratio, kind):
    """A shift removes the offset of a column (the contract of the shifted representations): 1e-9
    at every mean / sd.  Raw moments cancel (mean / sd)^2 of their digits: asserted up to 1e2,
    measured and printed beyond (DESIGN.md records the figures)."""
    X, y, ref = _offset(p, ratio)
    beta, nobs, rank = _solve([R.moments(X, y, kind)], p)
    assert nobs[0] == len(y)
    what = f"offset p={p} mean/sd={ratio:g} {kind}"
    if kind == "raw" and ratio > 1e2:
        e, es = _errors(beta[0], ref, X, np.arange(p))
        print(f"{what}: rank {rank[0]}, rel err {e:.3e}, slopes in sd units {es:.3e} "
              f"(measured, not asserted)")
        return
    assert rank[0] == p
    _check(beta[0], ref, X, np.arange(p), what)
