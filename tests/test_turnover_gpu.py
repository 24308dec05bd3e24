"""The stability statistics through screen_grid, FactorScreen and Pipeline.factor_screen
(afm/turnover.py, afm/screen.py) against tests/turnover_ref.py on the screen's own rows: values bit
for bit, order and dtypes of the frames as documented."""
import numpy as np
import pandas as pd
import pytest

import turnover_ref as R
from helpers import same
from test_sharded import SPLIT

pytestmark = pytest.mark.gpu

LAGS = (1, 5)
NAMES = list("abcdef")
PLAIN_KEYS = {"ic", "stats", "ir_year", "nrows", "rows_idx", "dates_idx", "years", "year0"}
PLAIN_BUFS = {"fr", "sig", "scratch", "rows", "rows_idx", "nrows", "ic", "stats", "ir_year",
              "summary_scratch"}
TURNOVER_KEYS = {"rank_ac", "turnover_counts", "port_turnover", "turnover_stats"}


@pytest.fixture(scope="module")
def ragged():
    """60 dates, 40 ids, price rows with p = 0.92, factor rows a subset of them; 6 columns: 'a'
    clean, 'b' rounded (ties), 'c' with NaN and inf cells, 'd' constant, 'e' slow (a random walk
    over the dates), 'f' positive (a long-only book)."""
    rng = np.random.default_rng(23)
    T, A = 60, 40
    dates = np.asarray(np.busday_offset(np.datetime64("2019-03-04"), np.arange(T), roll="forward"),
                       dtype="datetime64[ns]")
    ids = 500 + 7 * np.arange(A)
    present = rng.random((T, A)) < 0.92
    close = 30 * np.exp(np.cumsum(rng.normal(0, 0.02, (T, A)), axis=0))
    inframe = present & (rng.random((T, A)) < 0.9)
    F = rng.normal(size=(6, T, A))
    F[1] = np.round(F[1], 1)
    F[2][rng.random((T, A)) < 0.1] = np.nan
    F[2][rng.random((T, A)) < 0.03] = np.inf
    F[3] = 1.5
    F[4] = np.cumsum(rng.normal(0, 0.3, (T, A)), axis=0) + rng.normal(size=A)
    F[5] = np.abs(F[5]) + 0.5
    tt, aa = np.nonzero(inframe)
    df = pd.DataFrame({c: F[j, tt, aa] for j, c in enumerate(NAMES)},
                      index=pd.MultiIndex.from_arrays([dates[tt], ids[aa]]))
    pt, pa = np.nonzero(present)
    price = pd.DataFrame({"close_price": close[pt, pa]},
                         index=pd.MultiIndex.from_arrays([dates[pt], ids[pa]]))
    return df, price


def frame_planes(df, res):
    """The frame's columns as planes [K][T][lda] on the screen's calendar (res['dates'], ['ids'])."""
    T, lda = res["rows_idx"].shape
    fd = df.reset_index()
    t = np.searchsorted(res["dates"], fd[fd.columns[0]].to_numpy().astype("datetime64[ns]"))
    a = np.searchsorted(res["ids"], fd[fd.columns[1]].to_numpy().astype(np.int64))
    cols = list(df.columns)
    vals = np.full((len(cols), T, lda), np.nan)
    vals[:, t, a] = df[cols].to_numpy(np.float64).T
    return vals


def reference(vals, res, lags=LAGS):
    rows_idx, nrows = res["rows_idx"].cpu().numpy(), res["nrows"].cpu().numpy()
    return R.turnover(vals, rows_idx, nrows, res["dates_idx"], lags)


def check_frames(fs, ref, names, lags=LAGS):
    """turnover_df and turnover_summary of ``fs`` against the reference arrays."""
    ac, cnt, pt = ref
    nd, K, L = ac.shape
    dts = fs._res["dates"][fs._res["dates_idx"]]
    want = [(dts[i], names[k], lag, ac[i, k, l], cnt[i, k, l], pt[i, k, l])
            for i in range(nd) for k in range(K) for l, lag in enumerate(lags) if i >= lag]
    df = fs.turnover_df
    assert list(df.columns) == ["date", "factor", "lag", "rank_autocorr", "top_turnover",
                                "bottom_turnover", "port_turnover", "n_joint"]
    assert [str(t) for t in df.dtypes] == ["datetime64[ns]", "object", "int64", "float64",
                                           "float64", "float64", "float64", "int64"]
    assert len(df) == len(want) > 0
    assert same(df["date"].values.astype(np.int64),
                np.array([w[0] for w in want]).astype("datetime64[ns]").astype(np.int64))
    assert list(df["factor"]) == [w[1] for w in want] and list(df["lag"]) == [w[2] for w in want]
    assert same(df["rank_autocorr"].values, np.array([w[3] for w in want]))
    assert same(df["port_turnover"].values, np.array([w[5] for w in want]))
    c = np.array([w[4] for w in want], dtype=np.float64)
    with np.errstate(all="ignore"):
        assert same(df["top_turnover"].values, np.where(c[:, 1] > 0, c[:, 2] / c[:, 1], np.nan))
        assert same(df["bottom_turnover"].values, np.where(c[:, 3] > 0, c[:, 4] / c[:, 3], np.nan))
    assert same(df["n_joint"].values, c[:, 0].astype(np.int64))
    st = R.summary(ac, cnt, pt)                             # [K][L][4][2]
    key = st[:, 0, 3, 1]
    order = sorted(range(K), key=lambda k: (np.isnan(key[k]), key[k] if key[k] == key[k] else 0, k))
    sm = fs.turnover_summary
    assert list(sm.columns)[:7] == ["factor", "lag", "n", "rank_autocorr", "top_turnover",
                                    "bottom_turnover", "port_turnover"]
    assert list(sm["factor"]) == [names[k] for k in order for _ in lags]
    assert list(sm["lag"]) == list(lags) * K and str(sm["n"].dtype) == "int64"
    assert same(sm["n"].values, np.array([st[k, l, 0, 0] for k in order for l in range(L)]))
    for s, name in enumerate(["rank_autocorr", "top_turnover", "bottom_turnover", "port_turnover"]):
        assert same(sm[name].values, np.array([st[k, l, s, 1] for k in order for l in range(L)]))
    return st, order


def test_factor_screen_frames_equal_the_reference(ragged):
    import afm
    df, price = ragged
    spec = afm.Turnover(LAGS)
    fs = afm.FactorScreen(df.copy(), price.copy(), turnover=spec).run()
    vals = frame_planes(df, fs._res)
    ref = reference(vals, fs._res)
    assert len(fs._res["dates_idx"]) > 45
    st, order = check_frames(fs, ref, NAMES)
    assert "breakeven_cost" not in fs.turnover_summary
    assert not hasattr(fs, "composite_turnover_summary")
    # what the numbers say: the random walk keeps its ranks and its book, the noise does not
    m = fs.turnover_summary.set_index(["factor", "lag"])
    assert m.loc[("e", 1), "rank_autocorr"] > 0.8 > 0.3 > abs(m.loc[("a", 1), "rank_autocorr"])
    assert m.loc[("e", 1), "port_turnover"] < m.loc[("a", 1), "port_turnover"]
    assert np.isnan(m.loc[("d", 1), "rank_autocorr"]) and m.loc[("d", 1), "n"] == 0
    # the frame-level call
    tdf, tsm = afm.factor_turnover(df.copy(), price.copy(), columns=["e", "b"], lags=[1, 5])
    sub = fs.turnover_df[fs.turnover_df["factor"].isin(["e", "b"])]
    for c in ("rank_autocorr", "top_turnover", "bottom_turnover", "port_turnover", "n_joint"):
        for f in ("e", "b"):
            assert same(tdf[tdf["factor"] == f][c].values, sub[sub["factor"] == f][c].values)
    assert list(tdf["factor"][:2]) == ["e", "b"] and list(tdf["lag"][:2]) == [1, 1]
    assert set(tsm["factor"]) == {"e", "b"}


def test_screen_grid_results_and_turnover_none_changes_nothing(ragged):
    import torch
    import afm
    df, price = ragged
    fs = afm.FactorScreen(df.copy(), price.copy()).run()
    res = fs._res
    assert set(res) == PLAIN_KEYS | {"dates", "ids"}
    vals = frame_planes(df, res)
    T, lda = res["rows_idx"].shape
    dev = torch.device("cuda", 0)
    base = torch.from_numpy(vals).to(dev)
    fd, pd_ = df.reset_index(), price.reset_index()

    def mask_of(frame):
        t = np.searchsorted(res["dates"], frame[frame.columns[0]].to_numpy().astype("datetime64[ns]"))
        a = np.searchsorted(res["ids"], frame[frame.columns[1]].to_numpy().astype(np.int64))
        m = torch.zeros((T, lda), dtype=torch.bool, device=dev)
        m[torch.from_numpy(t).to(dev), torch.from_numpy(a).to(dev)] = True
        return m, t, a
    rm, _, _ = mask_of(fd)
    pm, ptt, pa = mask_of(pd_)
    close = torch.full((T, lda), float("nan"), dtype=torch.float64, device=dev)
    close[torch.from_numpy(ptt).to(dev), torch.from_numpy(pa).to(dev)] = \
        torch.from_numpy(pd_["close_price"].to_numpy(np.float64)).to(dev)
    args = (base, np.arange(len(NAMES)), close, afm.pack_bits(pm), afm.pack_bits(rm))
    bufs = {}
    plain = afm.screen_grid(*args, A=len(res["ids"]), bufs=bufs)
    assert set(plain) == PLAIN_KEYS and set(bufs) == PLAIN_BUFS
    assert same(plain["ic"].cpu().numpy(), res["ic"].cpu().numpy())
    spec = afm.Turnover(LAGS)
    got = afm.screen_grid(*args, A=len(res["ids"]), bufs=bufs, turnover=spec)
    assert set(got) == PLAIN_KEYS | TURNOVER_KEYS
    assert set(bufs) == PLAIN_BUFS | TURNOVER_KEYS | {"turnover_scratch"}
    assert same(got["ic"].cpu().numpy(), res["ic"].cpu().numpy())
    ac, cnt, pt = reference(vals, got)
    assert same(got["rank_ac"].cpu().numpy(), ac)
    assert got["turnover_counts"].dtype == torch.int32
    assert same(got["turnover_counts"].cpu().numpy(), cnt)
    assert same(got["port_turnover"].cpu().numpy(), pt)
    assert same(got["turnover_stats"].cpu().numpy(), R.summary(ac, cnt, pt))
    # the stand-alone call on the screen's rows gives the same
    alone = afm.turnover_grid(base, np.arange(len(NAMES)), got["rows_idx"], got["nrows"],
                              got["dates_idx"], T=T, lda=lda, spec=spec)
    for k in TURNOVER_KEYS:
        assert same(alone[k].cpu().numpy(), got[k].cpu().numpy()), k
    with pytest.raises(ValueError, match="ascending"):
        afm.turnover_grid(base, [0], got["rows_idx"], got["nrows"], got["dates_idx"][::-1].copy(),
                          T=T, lda=lda, spec=spec)
    with pytest.raises(ValueError, match="ascending"):
        afm.screen_grid(*args, A=len(res["ids"]), turnover=spec,
                        dates_idx=got["dates_idx"][::-1].copy())
    with pytest.raises(TypeError):
        afm.screen_grid(*args, A=len(res["ids"]), turnover=(1, 5))


def test_prep_is_the_turnover_of_the_preprocessed_frame(ragged):
    import afm
    df, price = ragged
    spec, prep = afm.Turnover(LAGS), afm.XsPrep("mad")
    cols = ["a", "b", "c", "e"]
    fs = afm.FactorScreen(df.copy(), price.copy(), columns=cols, prep=prep, turnover=spec).run()
    pre = afm.preprocess_factors(df.copy(), columns=cols, prep=prep)
    two = afm.FactorScreen(pre, price.copy(), columns=cols, turnover=spec).run()
    assert len(fs.turnover_df) == len(two.turnover_df) > 0
    for a, b in ((fs.turnover_df, two.turnover_df), (fs.turnover_summary, two.turnover_summary)):
        assert list(a.columns) == list(b.columns)
        for c in a.columns:
            assert same(a[c].to_numpy(), b[c].to_numpy()), c
    check_frames(two, reference(frame_planes(pre[cols], two._res), two._res), cols)


def test_combine_rates_the_composite_plane(ragged):
    import afm
    df, price = ragged
    spec = afm.Turnover(LAGS)
    comb = afm.ICWeights("ic", window=5, min_periods=2)
    fs = afm.FactorScreen(df.copy(), price.copy(), combine=comb, turnover=spec).run()
    r = fs._res
    T, lda = r["rows_idx"].shape
    alone = afm.turnover_grid(r["composite"], [0], r["rows_idx"], r["nrows"], r["dates_idx"], T=T,
                              lda=lda, spec=spec)
    for k in TURNOVER_KEYS:
        assert same(r["composite_" + k].cpu().numpy(), alone[k].cpu().numpy()), k
    comp = r["composite"].cpu().numpy()[None]
    ac, cnt, pt = reference(comp, r)
    assert same(r["composite_rank_ac"].cpu().numpy(), ac) and np.isfinite(ac[10:, 0, 0]).mean() > 0.9
    assert same(r["composite_turnover_counts"].cpu().numpy(), cnt)
    assert same(r["composite_port_turnover"].cpu().numpy(), pt)
    st = R.summary(ac, cnt, pt)
    cs = fs.composite_turnover_summary
    assert list(cs.columns) == ["lag", "n", "rank_autocorr", "top_turnover", "bottom_turnover",
                                "port_turnover"]
    assert list(cs["lag"]) == list(LAGS) and same(cs["n"].values, st[0, :, 0, 0].astype(np.int64))
    assert same(cs["port_turnover"].values, st[0, :, 3, 1])
    # the columns' own results are those without the composite
    check_frames(fs, reference(frame_planes(df, r), r), NAMES)


def test_breakeven_cost_is_the_mean_return_over_the_mean_turnover(ragged):
    import afm
    df, price = ragged
    fs = afm.FactorScreen(df.copy(), price.copy(), layers=True, turnover=afm.Turnover(LAGS)).run()
    st, order = check_frames(fs, reference(frame_planes(df, fs._res), fs._res), NAMES)
    port = fs._res["port"].cpu().numpy()[:, :, 0]
    sm = fs.turnover_summary
    assert list(sm.columns)[-1] == "breakeven_cost"
    want = []
    for k in order:
        v = port[:, k][~np.isnan(port[:, k])]
        with np.errstate(all="ignore"):
            want += [np.float64(v.mean()) / st[k, 0, 3, 1] if len(v) else np.nan, np.nan]
    assert same(sm["breakeven_cost"].values, np.array(want))
    assert np.isfinite(sm["breakeven_cost"].values[::2]).sum() >= 4
    later = afm.FactorScreen(df.copy(), price.copy(), layers=True, turnover=afm.Turnover((2, 5))).run()
    assert "breakeven_cost" not in later.turnover_summary    # needs lag 1


def test_pipeline_factor_screen_turnover():
    import torch
    import afm
    from afm import _lib
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.synthetic import make_panel
    torch.cuda.set_device(0)
    grid = afm.PanelGrid.from_panel(make_panel(300, 700, seed=11, tradable_p=0.9))
    pipe = Pipeline(grid, PipelineConfig(**SPLIT))
    pipe.step()
    torch.cuda.synchronize()
    spec = afm.Turnover((1, 5, 21))
    plain = pipe.factor_screen()
    assert not TURNOVER_KEYS & set(plain)
    got = pipe.factor_screen(turnover=spec)
    assert set(got) == set(plain) | TURNOVER_KEYS
    sp, lda, nch = pipe.sp, pipe.lda, pipe.nch
    rb, pb = torch.zeros_like(pipe.zrows), torch.zeros_like(pipe.alldf)
    _lib.run("afm_row_bits", nch, lda, pipe.zrows, None, None, 0, sp.tr1, rb)
    _lib.run("afm_row_bits", nch, lda, pipe.alldf, None, None, 0, sp.tr1, pb)
    hand = afm.screen_grid(pipe.out, pipe.feat, grid.close, pb, rb, A=grid.A, zs=pipe.zs,
                           turnover=spec)
    assert same(got["ic"], plain["ic"]) and same(got["ic"], hand["ic"].cpu().numpy())
    nd, K = got["ic"].shape[:2]
    assert got["rank_ac"].shape == (nd, K, 3) and got["turnover_counts"].shape == (nd, K, 3, 5)
    for k in TURNOVER_KEYS:
        assert same(got[k], hand[k].cpu().numpy()), k
    assert np.isfinite(got["rank_ac"][21:]).mean() > 0.9
    assert (got["turnover_stats"][:, :, 0, 0] > 50).mean() > 0.9
