"""tests/xsprep_ref.py pinned on the CPU: the float64 restatement equals direct pandas one-liners
on a small frame, the written-out quantile lerp equals np.quantile bit for bit (numpy is the
reference: pandas' own Series.quantile differs from it in the last bit on some inputs), and E64 --
the distance of the float64 restatement from the long-double one, the yardstick of the GPU tests'
tolerance -- is what the conditioning of each column family says."""
import numpy as np
import pandas as pd

import xsprep_ref as X
from helpers import same


def small_frame():
    rng = np.random.default_rng(5)
    T, A = 6, 37
    dates = pd.date_range("2020-01-01", periods=T)
    tt, aa = np.nonzero(rng.random((T, A)) < 0.8)
    df = pd.DataFrame({"x": rng.normal(size=len(tt)), "y": 1e6 + rng.normal(size=len(tt))},
                      index=pd.MultiIndex.from_arrays([dates[tt], aa], names=["date", "id"]))
    df.loc[df.index[::11], "x"] = np.nan
    df.loc[df.index[5::17], "x"] = np.inf
    sector = pd.Series(rng.integers(0, 4, size=A)[aa], index=df.index)
    return df, sector


def by_item(df, sector, col, winsor, p_lo, p_hi, flags):
    """The restatement item by item -> a Series on the frame's index."""
    out = pd.Series(np.nan, index=df.index)
    for d, rows in df.groupby(level="date"):
        it = X.item(rows[col].to_numpy(), sector.loc[rows.index].to_numpy(), 4, winsor, p_lo, p_hi,
                    flags)
        out.loc[rows.index] = it["out64"]
    return out


def test_restatement_equals_pandas_one_liners():
    df, sector = small_frame()
    for col in ("x", "y"):
        s = df[col].replace([np.inf, -np.inf], np.nan).dropna()
        g = s.groupby(level="date")
        # MAD winsorising
        med = g.transform("median")
        mad = (s - med).abs().groupby(level="date").transform("median")
        w = s.clip(med - X.MAD_C * mad, med + X.MAD_C * mad)
        got = by_item(df, sector, col, 1, X.MAD_C, X.MAD_C, 0)
        assert same(got.loc[s.index].to_numpy(), w.to_numpy()) and got.drop(s.index).isna().all()
        # quantile winsorising
        w2 = s.clip(g.transform(lambda v: np.quantile(v, 0.1)),
                    g.transform(lambda v: np.quantile(v, 0.9)))
        got = by_item(df, sector, col, 2, 0.1, 0.9, 0)
        assert same(got.loc[s.index].to_numpy(), w2.to_numpy())
        # sector neutralisation, then the z-score across the date
        sec = sector.loc[s.index]
        v = w - w.groupby([w.index.get_level_values("date"), sec.to_numpy()]).transform("mean")
        got = by_item(df, sector, col, 1, X.MAD_C, X.MAD_C, X.NEUTRALIZE)
        assert same(got.loc[s.index].to_numpy(), v.to_numpy())
        z = v.groupby(level="date").transform(lambda d: (d - d.mean()) / d.std())
        got = by_item(df, sector, col, 1, X.MAD_C, X.MAD_C, X.NEUTRALIZE | X.STANDARDIZE)
        assert same(got.loc[s.index].to_numpy(), z.to_numpy())
        z0 = g.transform(lambda d: (d - d.mean()) / d.std())
        got = by_item(df, sector, col, 0, 0, 0, X.STANDARDIZE)
        assert same(got.loc[s.index].to_numpy(), z0.to_numpy())


def test_quantile_lerp_is_numpy_bit_for_bit():
    rng = np.random.default_rng(8)
    cases = 0
    for n in (1, 2, 3, 4, 5, 7, 10, 63, 64, 100, 513):
        for kind in range(3):
            x = rng.normal(size=n)
            if kind == 1:
                x = np.round(x, 1)                                  # ties
            if kind == 2:
                x = 1e6 + x                                         # an offset
            s = np.sort(x)
            for q in (0.0, 0.01, 0.05, 0.1, 0.25, 1 / 3, 0.5, 0.75, 0.9, 0.95, 0.99, 1.0):
                want = np.quantile(x, q)
                assert X.quantile_lerp(s, q) == want, (n, kind, q)
                cases += 1
    assert cases == 11 * 3 * 12


def test_special_items():
    """mad == 0 leaves the column alone; a group of one row is exactly 0; n < 2 and a constant
    column standardise to NaN; a label outside [0, G) is a missing cell under neutralisation."""
    x = np.array([50.0, 50.0, 50.0, 50.0, 7.0, 90.0, 50.0])
    it = X.item(x, None, 0, 1, X.MAD_C, X.MAD_C, 0)
    assert same(it["out64"], x) and it["info64"][1] == -np.inf and it["info64"][2] == np.inf
    assert it["info64"][3] == 0 and it["info64"][4] == 0
    g = np.array([0, 0, 1, 2, 2, 2, 5])
    it = X.item(x, g, 3, 0, 0, 0, X.NEUTRALIZE)
    assert it["out64"][2] == 0.0 and np.isnan(it["out64"][6]) and it["info64"][0] == 6
    assert X.item(x, g, 3, 0, 0, 0, 0)["info64"][0] == 7
    for xs in (np.array([3.0]), np.full(9, 1.5)):
        for key in ("out64", "outld"):
            assert np.isnan(X.item(xs, None, 0, 0, 0, 0, X.STANDARDIZE)[key]).all()
    it = X.item(np.array([1.0, np.nan, 4.0, np.inf, 2.0, 3.0, 100.0]), None, 0, 2, 0.0, 0.8, 0)
    fin = np.array([1.0, 4.0, 2.0, 3.0, 100.0])
    assert it["info64"].tolist()[:5] == [5, 1.0, np.quantile(fin, 0.8), 0, 1]
    assert 4.0 < it["info64"][2] < 100.0 and same(it["out64"][[0, 2, 4, 5]], fin[:4])
    empty = X.item(np.array([np.nan, np.inf]), None, 0, 1, X.MAD_C, X.MAD_C, X.STANDARDIZE)
    assert empty["info64"][0] == 0 and np.isnan(empty["info64"][1:3]).all()
    assert np.isnan(empty["out64"]).all()


def test_E64_per_family():
    """E64 of every family of the shared inputs (the 513-row date, seven groups, MAD + neutralise +
    standardise): a few ulp of the output on the benign families, eps |mean| / sd on the
    1e6-offset one (standardise alone) -- and the tolerance never below its floor."""
    planes, rows_idx, nrows = X.small_case()
    t = X.SMALL_COUNTS.index(513)
    idx = rows_idx[t, :nrows[t]]
    g = X.group_labels(np.random.default_rng(1), (planes.shape[2],), 7)[idx]
    ulp1 = 2.0 ** -52
    for fam, name in enumerate(X.FAMILIES):
        it = X.item(planes[fam, t, idx], g, 7, 1, X.MAD_C, X.MAD_C, X.NEUTRALIZE | X.STANDARDIZE)
        alone = X.item(planes[fam, t, idx], None, 0, 0, 0, 0, X.STANDARDIZE)
        print(f"E64 {name}: full chain {it['E64']:.3e}, standardise alone {alone['E64']:.3e}")
        assert X.tolerance(it["E64"], it["outld"]) >= 16 * X.EPS
        if fam in (X.CONST, X.ALLMISS):
            assert np.isnan(it["outld"]).all() and it["E64"] == 0.0
        elif fam == X.OFFSET:
            assert 1e3 * ulp1 < alone["E64"] < 4e6 * ulp1      # ~ 2^-53 * 1e6 / sd, sd ~ 1
        else:
            assert it["E64"] <= 64 * ulp1 and alone["E64"] <= 64 * ulp1
    assert np.finfo(X.LD).nmant >= 63                          # a wider format than double
