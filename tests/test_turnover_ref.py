"""tests/turnover_ref.py -- the numpy / Python-int restatement of include/afm_turnover.h -- against
an independent pandas formulation (no GPU): groupby('date').rank() and Series.corr for the rank
autocorrelation, rank(method='first') and Python sets for the layers, rank(ascending=False,
method='first') <= 10 for the book."""
import math

import numpy as np
import pandas as pd
import pytest

import turnover_ref as R

T, A, LAGS = 40, 30, (1, 5)
COLS = ["a", "b", "c", "d"]


@pytest.fixture(scope="module")
def frame():
    rng = np.random.default_rng(20240607)
    x = rng.standard_normal((T, A, len(COLS)))
    x[:, :, 0] = np.round(x[:, :, 0] * 2) / 2              # heavy ties
    x[:, :8, 1] = np.round(x[:, :8, 1])                    # ties in a part of the names
    x[:, :, 3] = np.abs(x[:, :, 3]) + 0.1                  # a long-only book
    x[rng.random(x.shape) < 0.05] = np.nan
    present = rng.random((T, A)) < 0.85                    # holes: a ragged frame
    t, a = np.nonzero(present)
    dates = pd.date_range("2021-01-04", periods=T, freq="B")
    index = pd.MultiIndex.from_arrays([dates[t], 1000 + a], names=["date", "id"])
    return pd.DataFrame(x[t, a], index=index, columns=COLS), present, x


@pytest.fixture(scope="module")
def ref(frame):
    _, present, x = frame
    vals = np.ascontiguousarray(np.transpose(x, (2, 0, 1)))          # [K][T][A]
    rows_idx, nrows = R.rows_of(present)
    return R.turnover(vals, rows_idx, nrows, np.arange(T), LAGS)


def test_rank_autocorrelation_is_the_pearson_correlation_of_the_per_date_ranks(frame, ref):
    df, _, _ = frame
    ac = ref[0]
    finite = items = 0
    for k, c in enumerate(COLS):
        ranks = df[c].groupby(level="date").rank().unstack("id")     # NaN: no rank / not a row
        for l, lag in enumerate(LAGS):
            for i in range(lag, T):
                want = ranks.iloc[i].corr(ranks.iloc[i - lag])
                got = ac[i, k, l]
                items += 1
                if math.isnan(got):
                    assert math.isnan(want), (c, lag, i, want)
                else:
                    finite += 1
                    assert abs(got - want) <= 1e-12, (c, lag, i, got, want)
            assert np.isnan(ac[:lag, k, l]).all()
    assert finite >= 0.9 * items


def test_layer_counts_are_the_set_differences_of_rank_first_layers(frame, ref):
    df, _, _ = frame
    counts = ref[1]
    dates = df.index.get_level_values("date").unique()
    for k, c in enumerate(COLS):
        col = df[c].dropna()
        first = col.groupby(level="date").rank(method="first")
        nk = col.groupby(level="date").transform("size")
        layer = np.minimum((first / nk * 10).astype(int) + 1, 10)

        def ids_by_date(s):
            return {d: set(g.index.get_level_values("id")) for d, g in s.groupby(level="date")}
        ranked, top, bot = ids_by_date(col), ids_by_date(layer[layer == 10]), \
            ids_by_date(layer[layer == 1])
        for d in dates:
            assert top.get(d), (c, d)                      # every date has a layer 10
        for l, lag in enumerate(LAGS):
            for i in range(T):
                d1 = dates[i]
                if i < lag:
                    assert (counts[i, k, l] == 0).all()
                    continue
                d0 = dates[i - lag]
                t1, t0 = top.get(d1, set()), top.get(d0, set())
                b1, b0 = bot.get(d1, set()), bot.get(d0, set())
                want = [len(ranked.get(d1, set()) & ranked.get(d0, set())), len(t1), len(t1 - t0),
                        len(b1), len(b1 - b0)]
                assert counts[i, k, l].tolist() == want, (c, lag, i)


def test_port_turnover_is_half_the_absolute_weight_change_of_the_top_book(frame, ref):
    df, _, _ = frame
    turn = ref[2]
    dates = df.index.get_level_values("date").unique()
    for k, c in enumerate(COLS):
        col = df[c].dropna()
        desc = col.groupby(level="date").rank(ascending=False, method="first")
        held = col[desc <= 10]
        w = {d: (g / g.sum()).droplevel("date") for d, g in held.groupby(level="date")}
        for l, lag in enumerate(LAGS):
            for i in range(lag, T):
                w1, w0 = w.get(dates[i]), w.get(dates[i - lag])
                got = turn[i, k, l]
                if w1 is None or w0 is None or not (np.isfinite(w1).all() and np.isfinite(w0).all()):
                    assert math.isnan(got), (c, lag, i)
                    continue
                want = 0.5 * w1.sub(w0, fill_value=0.0).abs().sum()
                tol = 64 * 2.0 ** -53 * (w0.abs().sum() + w1.abs().sum())
                assert abs(got - want) <= tol, (c, lag, i, got, want)
            assert np.isnan(turn[:lag, k, l]).all()


def test_summary_is_the_mean_over_the_non_nan_dates(ref):
    ac, counts, turn = ref
    stats = R.summary(ac, counts, turn)
    assert stats.shape == (len(COLS), len(LAGS), 4, 2)
    with np.errstate(all="ignore"):
        series = [ac, np.where(counts[..., 1] > 0, counts[..., 2] / counts[..., 1], np.nan),
                  np.where(counts[..., 3] > 0, counts[..., 4] / counts[..., 3], np.nan), turn]
    for s, v in enumerate(series):
        n = (~np.isnan(v)).sum(axis=0)
        assert (stats[:, :, s, 0] == n).all()
        assert np.allclose(stats[:, :, s, 1], np.nanmean(v, axis=0), rtol=1e-13, atol=0)
    empty = R.summary(np.full((3, 1, 1), np.nan), np.zeros((3, 1, 1, 5), np.int32),
                      np.full((3, 1, 1), np.nan))
    assert (empty[..., 0] == 0).all() and np.isnan(empty[..., 1]).all()


def test_identical_dates_and_special_values():
    v = np.array([[3.0, -0.0, 0.0, np.inf, -np.inf, np.nan, 1.0, 1.0] + [np.nan] * 56])
    idx = np.arange(8)
    m = R.marks(v[0], idx)
    assert m[4] == 7 and m[0][5] == 0                      # the NaN has no rank
    assert m[0][1] == m[0][2] == 2 * 2.5                   # -0.0 ties with 0.0
    assert m[0][3] == 14 and m[0][4] == 2                  # +-inf are ranked
    ac, counts, turn = R.pair(m, m)
    assert ac == 1.0 and counts == [7, len(m[1]), 0, len(m[2]), 0]
    assert math.isnan(turn)                                # an infinite weight
    flat = R.marks(np.full(64, 2.0), np.arange(12))
    ac, counts, turn = R.pair(flat, flat)
    assert math.isnan(ac) and counts[0] == 12 and turn == 0.0
