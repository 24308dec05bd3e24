"""tests/rank_ref.py's integer restatement of the rank (Spearman) IC against the reference's own
statement -- DataFrame.corr(method='spearman') per date (KKT:344-345 with corr_method =
'spearman') -- bit for bit, NaN equal to NaN, on the CPU.  The GPU tests then hold the kernels to
the restatement."""
import numpy as np
import pandas as pd
import pytest

import rank_ref as K
from helpers import same

SIZES = (1, 2, 3, 64, 65, 2049, 9600)


def calc_sdav_ic(df: pd.DataFrame, corr_method: str) -> pd.DataFrame:
    """The reference's per-date IC (KKT:342-349) in pandas calls: per date the correlation matrix
    of [factor, returns], the factor's column without its own row, stacked."""
    ic = df.groupby("date").apply(lambda x: x[["f"] + K.RETURNS].corr(method=corr_method)["f"])
    return ic.drop(columns="f").stack().reset_index(name="IC")


@pytest.mark.parametrize("rkind", K.RETURN_KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_restatement_equals_pandas(n, rkind):
    """Every factor kind (no ties, heavy ties, two values, constant, signed zeros, +-inf / NaN in
    the factor only, +-inf / NaN on the rows where return_1 is not finite either) against finite
    returns, +-inf in return_2 only, and return_1 not finite on the special rows."""
    rng = np.random.default_rng(1000 * n + len(rkind))
    rets = K.return_values(rng, n, rkind)
    seen_nan = False
    for kind in K.FACTOR_KINDS:
        f = K.factor_values(rng, n, kind)
        want = K.ic_pandas(f, rets)
        got = K.ic_int(f, rets)
        assert same(got, want), (kind, got, want)
        seen_nan |= bool(np.isnan(got).any())
    assert seen_nan                                        # the constant column at least
    if n >= 64 and rkind == "fin":
        f = K.factor_values(rng, n, "ties")
        assert not np.isnan(K.ic_int(f, rets)).any()
        assert len(np.unique(f)) < n // 2                  # the ties are heavy


def test_quirk_keeps_the_rankings_of_the_whole_columns():
    """Both columns not finite on exactly the same rows: pandas keeps the rankings that include the
    +-inf rows and the mean (nobs + 1) / 2 -- not what ranking the common rows again gives."""
    rng = np.random.default_rng(5)
    n = 65
    rets = K.return_values(rng, n, "r1quirk")
    f = K.factor_values(rng, n, "quirk")
    got = K.ic_int(f, rets)
    assert same(got, K.ic_pandas(f, rets))
    m = np.isfinite(f) & np.isfinite(rets[0])
    again = K.ic_int(f[m], rets[:, m])
    assert got[0] != again[0]                              # return_1: the quirk
    assert same(got[1:], again[1:])                        # return_2 / 5: ranked again over m


def test_largest_date_and_the_exactness_bound():
    """n = 32,768: the doubled sums stay below 2^53 (so every one of pandas' float additions is
    exact, in any order), and the restatement still equals pandas."""
    n = K.MAX_ROWS
    rng = np.random.default_rng(9)
    rets = K.return_values(rng, n, "fin")
    f = np.round(rng.normal(size=n), 2)
    assert same(K.ic_int(f, rets), K.ic_pandas(f, rets))
    # the largest sums there can be: no ties, the two rankings equal
    r = np.arange(n, dtype=np.float64)
    nobs, sxy, sxx, syy = K.spearman_sums(r, r)
    assert nobs == n and sxy == sxx == syy == (n - 1) * n * (n + 1) // 3 < 2 ** 53
    # the quirk's ranks run past nobs: still far below
    f2 = r.copy()
    f2[:n // 2] = -np.inf
    nobs, sxy, sxx, syy = K.spearman_sums(f2, f2)
    assert nobs == n // 2 and max(sxy, sxx, syy) < 2 ** 53


def test_wide_frame_equals_the_pairs():
    """One corr() of [f_0 .. f_K-1, returns] gives each column's own entries: only the pair's
    masks enter, whatever the other columns hold."""
    rng = np.random.default_rng(3)
    for n, rkind in ((65, "r1quirk"), (130, "r2inf"), (64, "fin")):
        rets = K.return_values(rng, n, rkind)
        F = np.stack([K.factor_values(rng, n, kind) for kind in K.FACTOR_KINDS])
        wide = K.ic_pandas_wide(F, rets)
        for k in range(len(F)):
            assert same(wide[k], K.ic_pandas(F[k], rets)), K.FACTOR_KINDS[k]
            assert same(wide[k], K.ic_int(F[k], rets))


def test_reference_statement_per_date():
    """_calc_sdav_ic in pandas calls on a small frame: its Spearman ICs are the restatement's, its
    Pearson ICs are not."""
    rng = np.random.default_rng(11)
    recs = []
    for d, n in enumerate((30, 1, 47)):
        rets = K.return_values(rng, n, "fin")
        f = K.factor_values(rng, n, "ties")
        recs.append(pd.DataFrame(dict(zip(["f"] + K.RETURNS, [f, *rets]))).assign(date=d))
    df = pd.concat(recs, ignore_index=True)
    with np.errstate(all="ignore"):
        sp, pe = calc_sdav_ic(df, "spearman"), calc_sdav_ic(df, "pearson")
    want = np.concatenate([K.ic_int(g["f"].to_numpy(), g[K.RETURNS].to_numpy().T)
                           for _, g in df.groupby("date")])
    want = want[~np.isnan(want)]                           # stack() drops the one-row date
    assert len(want) == 6 and same(sp["IC"].to_numpy(), want)
    assert not same(pe["IC"].to_numpy(), want)
