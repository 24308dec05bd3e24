"""tests/layers_ref.py pinned on the CPU: restricting a date's rows to the column's non-NaN cells
and running the single-factor statements (analyzer_ref.stats_pandas) is what the reference's own
statements give on a frame that still holds the NaN cells -- ``rank`` leaves them without a rank,
so they have no layer and no place in the top 10 (KKT:328-332, 359-369)."""
import numpy as np
import pandas as pd

import analyzer_ref as R
import layers_ref as L
from helpers import same


def dates_with_nan(seed=5, counts=(30, 9, 12, 0, 57, 11)):
    """Per date (f [n], rets [3][n]): ties, NaN (a whole date of it, and a date left with fewer
    than ten rows) and +-inf in f; inf in a return."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(counts):
        f = np.round(rng.normal(size=n), 1)
        f[rng.random(n) < 0.25] = np.nan
        if n == 12:
            f[:] = np.nan
        if n == 57:
            f[[3, 40]] = [np.inf, -np.inf]
        rets = rng.normal(size=(3, n)) * 0.02
        if n == 30:
            rets[1, 4] = np.inf
        out.append((f, rets))
    return out


def statements_on_the_nan_frame(dates):
    """KKT:328-332 and 359-369 on frames that hold the NaN cells."""
    nd = len(dates)
    lm = np.full((nd, 3, 10), np.nan)
    lc = np.zeros((nd, 10), dtype=np.int32)
    frames = []
    for i, (f, rets) in enumerate(dates):
        df = pd.DataFrame(dict(zip(R.COLS, [f, *rets])))
        pct = df["f"].rank(pct=True, method="first")                   # NaN cells: NaN rank
        df = df[pct.notna()].copy()                                    # ... dropped before astype
        layer = (pct[pct.notna()] * 10).astype(int) + 1
        layer[layer > 10] = 10
        df["layer"] = layer
        with np.errstate(all="ignore"):
            for k, rt in enumerate(R.RETURNS):
                m = df.groupby("layer")[rt].mean()
                lm[i, k, m.index.to_numpy() - 1] = m.to_numpy()
        cnt = df.groupby("layer").size()
        lc[i, cnt.index.to_numpy() - 1] = cnt.to_numpy()
        full = pd.DataFrame(dict(zip(R.COLS, [f, *rets])))
        full["date"] = i
        frames.append(full)
    pdf = pd.concat(frames, ignore_index=True)
    pdf["rank"] = pdf.groupby("date")["f"].rank(method="first", ascending=False)
    pdf = pdf[pdf["rank"] <= 10].sort_values(by=["date", "rank"])      # NaN <= 10 is False
    pdf["rank"] = pdf["rank"].astype(str)
    port = np.zeros((nd, 3))
    with np.errstate(all="ignore"):
        w = pd.pivot(data=pdf, index="date", columns="rank", values="f")
        w = w.div(w.sum(axis=1), axis=0)
        for k, rt in enumerate(R.RETURNS):
            ret = pd.pivot(data=pdf, index="date", columns="rank", values=rt)
            port[:, k] = ret.mul(w).sum(axis=1).reindex(range(nd)).to_numpy()
    return lm, lc, port


def test_restrict_is_the_identity_on_a_nan_free_column():
    rng = np.random.default_rng(3)
    f = np.round(rng.normal(size=40), 1)
    f[[2, 9]] = [np.inf, -np.inf]                          # inf is ranked: it stays
    rets = rng.normal(size=(3, 40))
    got = L.restrict(f, rets)
    assert same(got, np.stack([f, *rets]))
    a = R.stats_pandas([got])
    b = R.stats_pandas([np.stack([f, *rets])])
    assert all(same(x, y) for x, y in zip(a, b))


def test_restrict_equals_the_statements_on_the_nan_frame():
    dates = dates_with_nan()
    assert any(np.isnan(f).all() and len(f) for f, _ in dates)
    assert any(0 < (~np.isnan(f)).sum() < 10 for f, _ in dates)
    lm, lc, port = statements_on_the_nan_frame(dates)
    _, lm2, lc2, port2 = R.stats_pandas([L.restrict(f, r) for f, r in dates])
    assert same(lm, lm2) and same(lc, lc2) and same(port, port2)
    assert np.isnan(port[2]).all() and np.isnan(port[3]).all() and not np.isnan(port[0]).any()
    assert (lc[2] == 0).all() and lc[0].sum() == (~np.isnan(dates[0][0])).sum()


def test_layers_ref_shapes_and_empty_dates():
    """The wide reference on screen_ref's inputs: a date without rows and a column that is NaN on
    a whole date give layer_cnt 0 and NaN; the pivot of a column is joint over the dates."""
    counts = (0, 3, 63, 12)
    planes, rows, rows_idx, nrows = L.layer_inputs(counts, "inf")
    cols = [128, 0, 2]
    lm, lc, port = L.layers_ref(planes, rows, rows_idx, nrows, cols)
    assert lm.shape == (4, 3, 3, 10) and lc.shape == (4, 3, 10) and port.shape == (4, 3, 3)
    assert (lc[0] == 0).all() and np.isnan(lm[0]).all() and np.isnan(port[0]).all()
    assert (lc[2, 0] == 0).all() and np.isnan(port[2, 0]).all()     # plane 128: NaN on 63 rows
    assert lc[2, 1].sum() == 63 and lc[2, 2].sum() == 62 and lc[1, 1].sum() == 3
    sub = L.layers_ref(planes, rows, rows_idx, nrows, cols, dates=[3, 1])
    assert same(sub[0][0], lm[3]) and same(sub[1][1], lc[1])
    cum, ls, cp = L.series_ref(lm, port)
    assert cum.shape == lm.shape and ls.shape == (4, 3, 3, 5) and np.isnan(cp[0]).all()
    assert same(cp[1, 1], port[1, 1]) and same(cp[3, 1], port[1, 1] + port[2, 1] + port[3, 1])


def test_kernel_constants_are_readable():
    assert L.kernel_constant("kSlSelectRows") == (L.kernel_constant("kSlSmallKeys") *
                                                  L.kernel_constant("kSlThreads"))
    assert L.kernel_constant("kSlFewRows") == (L.kernel_constant("kSlFewKeys") *
                                               L.kernel_constant("kSlThreads"))
    edges = L.counts_edges()
    chunk = L.kernel_constant("kSlChunk")
    assert {9, 10, 11, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 3 * chunk - 1} <= set(edges)
