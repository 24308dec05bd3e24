"""tests/combine_ref.py against independent statements (no GPU): pandas' rolling mean / std for
methods 1 and 2, numpy.linalg.solve on the shrunk covariance for method 3, and the explicit
sum w x / sum |w| over a small frame for the composite."""
import numpy as np
import pandas as pd
import pytest

import combine_ref as R


def ic_panel(nd, K, seed, nan_frac=0.0, mu=0.02, sd=0.05):
    """ICs as a screen gives them: a small positive mean, a larger spread."""
    rng = np.random.default_rng(seed)
    ic = mu + sd * rng.standard_normal((nd, K, 3))
    if nan_frac:
        ic[rng.random((nd, K, 3)) < nan_frac] = np.nan
    return ic


def ulps(a, b):
    with np.errstate(all="ignore"):
        return np.abs(a - b) / np.spacing(np.abs(b))


def two_pass_std(x):
    x = x[~np.isnan(x)]
    return np.std(x, ddof=1) if len(x) > 1 else np.nan


@pytest.mark.parametrize("nan_frac", [0.0, 0.1])
@pytest.mark.parametrize("window,embargo,minp", [(5, 0, 2), (20, 1, 10), (20, 5, 20), (7, 2, 3)])
def test_rolling_mean_and_icir_match_pandas(window, embargo, minp, nan_frac):
    """Methods 1 and 2 against ``ic_df.rolling(window, min_periods).mean() / .std()`` shifted by
    the embargo, within 8 ulp of the value.

    "Of the value" needs a value that is no cancellation residue, so the ICs here have mean 0.05
    and sd 0.02: the mean of a window is then of the size of its terms (with mean 0.02, sd 0.05
    the two orders of summation already differ by 146 ulp of a mean near 0).  Measured on these
    cases: the mean within 5 ulp of pandas' on every position.

    pandas' rolling std is exact to a few ulp only while its window grows: once it removes an
    observation, the recurrence carries the rounding of earlier, larger sums of squares into a
    window of small spread -- against a long-double restatement pandas' own std is off by up to
    81 ulp (NaN-free) and 621 ulp (10 % NaN) on these cases, this file's by at most 5.  So
    ``.std()`` is the yardstick on the positions whose window has not yet dropped a date (i -
    embargo < window; measured: within 5 ulp), and on the positions after it the same pandas
    windows with a two-pass std are (measured: within 5 ulp).  That the window drops the right
    dates is what the mean, over the same J, shows on every position.

    Plain ``.std()`` is not dropped on the later positions either: there it is held to a bound of
    the recurrence's own error.  Each add or remove rounds a running sum of squared deviations
    that has been as large as SS_max, the largest any window of the column held so far; with at
    most two updates per date and four operations per update the variance of date t is off by at
    most 8 t u SS_max, i.e. the sd by a relative 4 t u SS_max / SS, SS the window's own sum.  So
    |restatement - pandas| <= (8 u + 4 t u SS_max / SS) |value|.  Measured: at most 0.13 of that
    bound."""
    nd, K, q = 60, 7, 1
    ic = ic_panel(nd, K, 11 + window, nan_frac, mu=0.05, sd=0.02)
    df = pd.DataFrame(ic[:, :, q])
    roll = df.rolling(window, min_periods=minp)
    mean = roll.mean().shift(embargo).to_numpy()
    icir = (roll.mean() / roll.std()).shift(embargo).to_numpy()
    icir2 = (roll.mean() / roll.apply(two_pass_std, raw=True)).shift(embargo).to_numpy()
    grows = np.broadcast_to(np.arange(nd)[:, None] - embargo < window, (nd, K))
    ss = roll.apply(lambda x: ((x[~np.isnan(x)] - x[~np.isnan(x)].mean()) ** 2).sum(), raw=True)
    t = np.arange(1, nd + 1)[:, None]
    with np.errstate(all="ignore"):
        loose = (8 * R.U + 4 * t * R.U * (ss.cummax() / ss)).shift(embargo).to_numpy()
    for method, want in ((R.IC, mean), (R.ICIR, icir)):
        raws = []
        w, info = R.ic_weights_ref(ic, q, method, window, embargo, minp, raws=raws)
        raw = np.array([r for r, _ in raws])
        act = np.array([a for _, a in raws])
        assert (act == ~np.isnan(want)).all()
        assert act.any() and (~act).any() and (act & grows).any() and (act & ~grows).any()
        if method == R.IC:
            assert ulps(raw[act], want[act]).max() <= 8
        else:
            assert ulps(raw[act & grows], want[act & grows]).max() <= 8
            assert ulps(raw[act & ~grows], icir2[act & ~grows]).max() <= 8
            late = act & ~grows
            rel = np.abs(raw[late] - want[late]) / np.abs(want[late])
            print(f"icir against plain .std() after a removal: at most {rel.max() / R.U:.0f} u, "
                  f"{(rel / loose[late]).max():.2f} of the recurrence's bound")
            assert (rel <= loose[late]).all()
        tot = np.abs(np.where(act, raw, 0)).sum(axis=1)
        have = act.any(axis=1)
        assert (np.isnan(w).all(axis=1) == ~have).all()
        want_w = np.where(act, raw, 0)[have] / tot[have, None]
        assert np.allclose(w[have], want_w, rtol=1e-14, atol=0)
        assert (info[:, 0] == act.sum(axis=1)).all()
        assert np.allclose(np.abs(w[have]).sum(axis=1), 1.0, rtol=1e-14)
    assert np.isnan(w[:embargo]).all()


def test_equal_weights_and_window():
    ic = ic_panel(9, 4, 3)
    w, info = R.ic_weights_ref(ic, 0, R.EQUAL, 5, 2, 2)
    assert (w == 0.25).all() and (info == [4, 0, 4]).all()
    assert list(R.window_of(1, 5, 2)) == [] and list(R.window_of(2, 5, 2)) == [0]
    assert list(R.window_of(8, 5, 2)) == [2, 3, 4, 5, 6]
    assert list(R.window_of(3, 1, 0)) == [3]


@pytest.mark.parametrize("K,window,shrink,nan_dates", [(3, 20, 0.5, False), (17, 20, 0.1, True),
                                                       (40, 30, 1.0, False), (65, 20, 0.25, True)])
def test_maxir_matches_numpy_solve(K, window, shrink, nan_dates):
    nd, q, embargo, minp = 45, 2, 1, 5
    ic = ic_panel(nd, K, 5 + K)
    if nan_dates:
        ic[[4, 9, 23]] = np.nan
        ic[30, 0] = np.nan
    ic[:, K - 1] = ic[:, 0]                                 # a copy: singular without the shrink
    systems, sys_ld = [], []
    w, info = R.ic_weights_ref(ic, q, R.MAXIR, window, embargo, minp, shrink, systems=systems)
    wl, il = R.ic_weights_ref(ic, q, R.MAXIR, window, embargo, minp, shrink, dtype=np.longdouble,
                              systems=sys_ld)
    assert (info[:, :2] == il[:, :2]).all()
    solved = 0
    for (i, a, D, A, m, x), (_, al, Dl, Al, ml, xl) in zip(systems, sys_ld):
        assert (a == al).all() and (D == Dl).all()
        J = np.array(list(R.window_of(i, window, embargo)), dtype=np.int64)
        Dn = np.array([j for j in J if np.isfinite(ic[j, :, q]).all()], dtype=np.int64)
        if len(Dn) < minp:
            assert not len(a) and np.isnan(w[i]).all()
            continue
        assert (D == Dn).all() and len(a) == K
        X = ic[D][:, :, q]
        S = np.cov(X.T, ddof=1).reshape(K, K)
        An = (1 - shrink) * S + shrink * np.diag(np.diag(S))
        xn = np.linalg.solve(An, X.mean(axis=0))
        cond = np.linalg.cond(An, np.inf)
        scale = np.abs(xn).max()
        assert np.abs(x - xn).max() <= 64 * cond * R.U * scale
        assert np.abs(np.asarray(xl, dtype=np.float64) - xn).max() <= 64 * cond * R.U * scale
        assert np.allclose(w[i], xn / np.abs(xn).sum(), rtol=0, atol=64 * cond * R.U)
        assert info[i, 0] == K and info[i, 1] == len(D)
        solved += 1
    assert solved >= nd // 2


def test_maxir_drops_a_column_without_variance_and_fails_on_a_bad_pivot():
    ic = ic_panel(30, 4, 9)
    ic[:, 2] = 0.25
    systems = []
    w, info = R.ic_weights_ref(ic, 0, R.MAXIR, 10, 0, 4, 0.5, systems=systems)
    assert (w[5:, 2] == 0).all() and (info[5:, 0] == 3).all() and (info[5:, 1] >= 6).all()
    assert np.isnan(w[:3]).all() and (info[:3, 0] == 0).all()
    assert R._cholesky_solve(np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones(2)) is None


def test_composite_matches_the_explicit_expression():
    rng = np.random.default_rng(2)
    T, lda, K = 5, 64, 4
    base = rng.standard_normal((K, T, lda))
    base[rng.random(base.shape) < 0.15] = np.nan
    base[1, 2, 5] = np.inf
    rows_idx = np.zeros((T, lda), dtype=np.int32)
    nrows = np.array([10, 0, 64, 1, 33], dtype=np.int32)
    for t in range(T):
        rows_idx[t, :nrows[t]] = np.sort(rng.permutation(lda)[:nrows[t]])
    w = rng.standard_normal((3, K))
    w[1, 2] = 0.0
    w[2] = np.nan
    dates = [4, 0, 2]
    sent = np.full((T, lda), -7.0)
    out, cnt = R.combine_ref(base, [0, 1, 2, 3], dates, rows_idx, nrows, w, sent,
                             np.full((T, lda), -7, dtype=np.int32))
    assert (out[[1, 3]] == -7.0).all() and (cnt[[1, 3]] == -7).all()
    assert np.isnan(out[2]).all() and (cnt[2] == 0).all()      # the NaN weight row
    for i, t in enumerate(dates[:2]):
        on = np.zeros(lda, dtype=bool)
        on[rows_idx[t, :nrows[t]]] = True
        x = base[:, t, :]
        use = np.isfinite(x) & (w[i] != 0)[:, None]
        num = np.where(use, w[i][:, None] * np.where(use, x, 0), 0).sum(axis=0)
        den = np.where(use, np.abs(w[i])[:, None], 0).sum(axis=0)
        with np.errstate(all="ignore"):
            want = np.where(on & (den > 0), num / den, np.nan)
        assert (np.isnan(out[t]) == np.isnan(want)).all()
        ok = ~np.isnan(want)
        assert np.allclose(out[t][ok], want[ok], rtol=1e-13, atol=1e-15)
        assert (cnt[t] == np.where(on, use.sum(axis=0), 0)).all()
    # one row of weights for every date; z on the fly; a repeat counts twice
    zs = np.stack([rng.standard_normal((K, lda)), 1.0 + rng.random((K, lda))], axis=2)
    o1, c1 = R.combine_ref(base, [0, 0], [0], rows_idx, nrows, np.array([0.5, 0.5]), sent, cnt)
    o2, _ = R.combine_ref(base, [0], [0], rows_idx, nrows, np.array([2.0]), sent, cnt)
    a = rows_idx[0, :nrows[0]]
    assert np.array_equal(o1[0, a], o2[0, a], equal_nan=True) and set(c1[0, a]) <= {0, 2}
    oz, _ = R.combine_ref(base, [1], [2], rows_idx, nrows, np.array([-3.0]), sent, cnt, zs=zs,
                          zcols=[3])
    z = (base[1, 2] - zs[3, :, 0]) * zs[3, :, 1]
    with np.errstate(all="ignore"):
        want = np.where(np.isfinite(z), -3.0 * z / 3.0, np.nan)
    assert np.array_equal(oz[2], want, equal_nan=True)
