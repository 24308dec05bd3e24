"""The layers / long-short / top-k half of the factor screen end to end: ``screen_grid(layers=
True)`` against the single-factor path it batches (``evaluate_grid``), ``FactorScreen(layers=
True)`` against ``AlphaSignalAnalyzer`` and the pandas statements on a ragged frame
(tests/layers_ref.py), and ``Pipeline.factor_screen(layers=True)`` on a stepped pipeline.  Bit for
bit, NaN equal to NaN."""
import numpy as np
import pandas as pd
import pytest

import analyzer_ref as R
import layers_ref as L
from helpers import same
from test_sharded import SPLIT

pytestmark = pytest.mark.gpu

LAYER_KEYS = ("layer_mean", "layer_cnt", "port", "cum_layer", "ls", "cum_port")
TODAY_KEYS = {"ic", "stats", "ir_year", "nrows", "rows_idx", "dates_idx", "years", "year0"}


def years_of(dates):
    return np.asarray(dates).astype("datetime64[Y]").astype(np.int64) + 1970


# ---- screen_grid(layers=True) == K calls of evaluate_grid ---------------------------------------------
def test_screen_grid_layers_equal_the_single_factor_path():
    """200 assets x 300 dates, 8 raw panel columns on the panel's NaN-free rows: for each column
    the analyzer's own layer means, counts, top-10 returns and their series are the screen's, bit
    for bit; the IC half of the same call is that of layers=False, and the backtests do not
    depend on corr_method."""
    import torch
    import afm
    from afm.analyzer import evaluate_grid
    from afm.factors import COL, factor_panel
    from afm.synthetic import make_panel
    torch.cuda.set_device(0)
    grid = afm.PanelGrid.from_panel(make_panel(200, 300, seed=3))
    out, nanfree = factor_panel(grid)
    names = ["SMA_6", "RSI_14", "MOM_20", "sd_5", "corr_15", "PSY", "OBV", "ROCR_32"]
    cols = np.array([COL[n] for n in names], np.int32)
    year = years_of(grid.dates)
    args = (out, cols, grid.close, grid.vbits, nanfree)
    plain = afm.screen_grid(*args, A=grid.A, year=year)
    assert set(plain) == TODAY_KEYS
    bufs = {}
    scr = afm.screen_grid(*args, A=grid.A, year=year, layers=True, bufs=bufs)
    assert set(scr) == TODAY_KEYS | set(LAYER_KEYS)
    assert all(bufs[k] is scr[k] for k in LAYER_KEYS)
    for k in ("ic", "stats", "ir_year"):
        assert same(scr[k].cpu().numpy(), plain[k].cpu().numpy()), k
    assert same(scr["dates_idx"], plain["dates_idx"])
    got = {k: scr[k].cpu().numpy() for k in LAYER_KEYS}
    nd = len(scr["dates_idx"])
    assert nd > 200 and got["layer_mean"].shape == (nd, 8, 3, 10) and got["ls"].shape == (nd, 8, 3, 5)
    assert got["layer_cnt"].dtype == np.int32 and not np.isnan(got["cum_layer"]).all()
    rowm = afm.unpack_bits(nanfree, grid.T)
    for k, c in enumerate(cols):
        sig = torch.where(rowm, out[c], torch.full_like(out[c], float("nan")))
        one = evaluate_grid(sig, grid.close, grid.vbits, A=grid.A, year=year)
        assert same(one["dates_idx"], scr["dates_idx"]) and one["mcols"] == 10
        for key in LAYER_KEYS:
            assert same(got[key][:, k], one[key].cpu().numpy()), (key, names[k])
    rank = afm.screen_grid(*args, A=grid.A, year=year, layers=True, corr_method="spearman")
    for key in LAYER_KEYS:
        assert same(rank[key].cpu().numpy(), got[key]), key
    assert not same(rank["ic"].cpu().numpy(), scr["ic"].cpu().numpy())


# ---- FactorScreen(layers=True) on a ragged frame ------------------------------------------------------
NAMES = list("abcde")


@pytest.fixture(scope="module")
def ragged():
    """The frame of tests/test_screen_gpu.py: 40 dates over two calendar years, 90 ids, price rows
    with p = 0.9, factor rows a subset of them; 5 columns: 'a' clean, 'b' rounded (ties), 'c' with
    NaN and inf cells, 'd' constant, 'e' = -a.  And the pandas statements per column on the same
    rows (tests/layers_ref.py): the arrays the frames are made of."""
    rng = np.random.default_rng(17)
    T, A = 40, 90
    dates = np.asarray(np.busday_offset(np.datetime64("2018-12-03"), np.arange(T), roll="forward"),
                       dtype="datetime64[ns]")
    ids = 1000 + 3 * np.arange(A)
    present = rng.random((T, A)) < 0.9
    close = 30 * np.exp(np.cumsum(rng.normal(0, 0.02, (T, A)), axis=0))
    inframe = present & (rng.random((T, A)) < 0.85)
    F = rng.normal(size=(5, T, A))
    F[1] = np.round(F[1], 1)
    F[2][rng.random((T, A)) < 0.1] = np.nan
    F[2][rng.random((T, A)) < 0.03] = np.inf
    F[3] = 1.5
    F[4] = -F[0]
    tt, aa = np.nonzero(inframe)
    df = pd.DataFrame({c: F[j, tt, aa] for j, c in enumerate(NAMES)},
                      index=pd.MultiIndex.from_arrays([dates[tt], ids[aa]]))
    pt, pa = np.nonzero(present)
    price = pd.DataFrame({"close_price": close[pt, pa]},
                         index=pd.MultiIndex.from_arrays([dates[pt], ids[pa]]))
    fr = R.fwd_returns_ref(np.where(present, close, np.nan), present)
    prep = R.prepare_ref(np.where(inframe, 0.0, np.nan), fr)
    didx = [t for t in range(T) if len(prep[t][0])]
    nd = len(didx)
    lm, lc, port = np.empty((nd, 5, 3, 10)), np.empty((nd, 5, 10), np.int32), np.empty((nd, 5, 3))
    for k in range(5):
        dr = [L.restrict(F[k, t, prep[t][0]], prep[t][1][1:]) for t in didx]
        _, lm[:, k], lc[:, k], port[:, k] = R.stats_pandas(dr)
    cum, ls, cp = L.series_ref(lm, port)
    return dict(df=df, price=price, dates=dates[didx], lm=lm, lc=lc, port=port, cum=cum, ls=ls,
                cp=cp)


def want_frames(g, q):
    """The analyzer's row rules (KKT:331-340) over the reference arrays: per date, factors in
    column order; the layers a factor has on any date, NaN entries dropped; long-short layer 5
    first."""
    lay, lsr = [], []
    for i, d in enumerate(g["dates"]):
        for k, name in enumerate(NAMES):
            for l in range(10):
                x = g["cum"][i, k, q, l]
                if (g["lc"][:, k, l] > 0).any() and x == x:
                    lay.append((d, name, l + 1, x))
            for j in range(5):
                x = g["ls"][i, k, q, j]
                if x == x:
                    lsr.append((d, name, 5 - j, x))
    return lay, lsr


def frame_is(df, want, columns):
    assert list(df.columns) == columns
    assert len(df) == len(want) > 0
    assert same(df["date"].values.astype(np.int64),
                np.array([w[0] for w in want]).astype("datetime64[ns]").astype(np.int64))
    assert list(df["factor"]) == [w[1] for w in want]
    assert list(df[columns[2]]) == [w[2] for w in want]
    assert same(df[columns[3]].values, np.array([w[3] for w in want], dtype=np.float64))


def test_factor_screen_layer_frames(ragged):
    """Every column against the pandas statements: 'c' leaves its NaN cells out and ranks its
    inf cells, 'd' (constant) has the position-ordered layers."""
    import afm
    g = ragged
    fs = afm.FactorScreen(g["df"].copy(), g["price"].copy(), layers=True).run()
    lc = g["lc"]
    assert (lc[:, 2].sum(axis=1) < lc[:, 0].sum(axis=1)).any()        # 'c' lost rows to NaN
    assert same(lc[:, 3], lc[:, 0]) and not same(g["lm"][:, 3], g["lm"][:, 0])
    for q, rt in enumerate(R.RETURNS):
        lay, lsr = want_frames(g, q)
        frame_is(fs.layered_ret_dfs[rt], lay, ["date", "factor", "layer", rt])
        frame_is(fs.ls_ret_dfs[rt], lsr, ["date", "factor", "layer", rt])
        assert fs.layered_ret_dfs[rt]["layer"].dtype == np.int64
    tn = list(R.RETURNS) + [f"cum_{x}" for x in R.RETURNS]
    full = np.concatenate([g["port"], g["cp"]], axis=2)
    want = [(d, name, tn[j], full[i, k, j]) for i, d in enumerate(g["dates"])
            for k, name in enumerate(NAMES) for j in range(6)]
    frame_is(fs.port_ret_df, want, ["date", "factor", "Type", "Returns"])
    # layer_summary: one row per (factor, Type), by |top_minus_bottom| descending, NaN last
    def last(x):
        x = x[~np.isnan(x)]
        return x[-1] if len(x) else np.nan
    rows = []
    for k, name in enumerate(NAMES):
        for q, rt in enumerate(R.RETURNS):
            fin = np.array([last(g["cum"][:, k, q, l]) for l in range(10)])
            have = ~np.isnan(fin)
            mono = pd.DataFrame({"l": np.arange(1, 11)[have], "v": fin[have]}).corr(
                method="spearman").iloc[0, 1]
            rows.append((name, rt, last(g["ls"][:, k, q, 0]), mono, last(g["cp"][:, k, q])))
    key = [abs(r[2]) for r in rows]
    order = sorted(range(15), key=lambda i: (np.isnan(key[i]), -key[i] if key[i] == key[i] else 0, i))
    ly = fs.layer_summary
    assert list(ly.columns) == ["factor", "Type", "top_minus_bottom", "monotonic", "top_k"]
    assert list(ly["factor"]) == [rows[i][0] for i in order]
    assert list(ly["Type"]) == [rows[i][1] for i in order]
    assert same(ly["top_minus_bottom"].values, np.array([rows[i][2] for i in order]))
    assert same(ly["top_k"].values, np.array([rows[i][4] for i in order]))
    # the host-side Spearman of at most ten ranks: two fp64 evaluations of the same quotient
    mono = np.array([rows[i][3] for i in order])
    assert same(np.isnan(ly["monotonic"].values), np.isnan(mono))
    assert np.allclose(ly["monotonic"].values, mono, rtol=0, atol=1e-12, equal_nan=True)
    assert np.abs(mono[~np.isnan(mono)]).max() <= 1 + 1e-12 and (~np.isnan(mono)).sum() == 15
    # the IC half is what it is without layers, and without layers there are no layer frames
    plain = afm.FactorScreen(g["df"].copy(), g["price"].copy()).run()
    assert plain.ic_df.equals(fs.ic_df) and plain.summary.equals(fs.summary)
    assert not hasattr(plain, "layer_summary") and not hasattr(plain, "port_ret_df")


@pytest.mark.parametrize("c", ["a", "b"])
def test_factor_screen_layer_frames_equal_the_analyzer(ragged, c):
    """A column without NaN: its rows of the frames are the single-factor analyzer's frames,
    values and row order."""
    import afm
    g = ragged
    fs = afm.FactorScreen(g["df"].copy(), g["price"].copy(), columns=["b", "a"], layers=True).run()
    an = afm.AlphaSignalAnalyzer(g["df"][[c]].copy(), c, g["price"].copy())
    an.run()

    def mine(df):
        return df[df["factor"] == c].drop(columns="factor").reset_index(drop=True)
    for rt in R.RETURNS:
        for got, one in ((mine(fs.layered_ret_dfs[rt]), an.layered_ret_dfs[rt]),
                         (mine(fs.ls_ret_dfs[rt]), an.ls_ret_dfs[rt])):
            assert list(got.columns) == list(one.columns) and len(got) == len(one) > 100
            assert same(got["date"].values.astype(np.int64), one["date"].values.astype(np.int64))
            assert same(got["layer"].values, one["layer"].values)
            assert same(got[rt].values, one[rt].values)
    got, one = mine(fs.port_ret_df), an.port_ret_df
    assert list(got.columns) == list(one.columns) and len(got) == len(one) > 100
    assert same(got["date"].values.astype(np.int64), one["date"].values.astype(np.int64))
    assert list(got["Type"]) == list(one["Type"])
    assert same(got["Returns"].values, one["Returns"].values)


# ---- Pipeline.factor_screen(layers=True) --------------------------------------------------------------
def test_pipeline_factor_screen_layers():
    import torch
    import afm
    from afm import _lib
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.sharded import EmulatedComm
    from afm.synthetic import make_panel
    torch.cuda.set_device(0)
    grid = afm.PanelGrid.from_panel(make_panel(300, 700, seed=11, tradable_p=0.9))
    pipe = Pipeline(grid, PipelineConfig(**SPLIT))
    pipe.step()
    torch.cuda.synchronize()
    before = pipe.summary()
    plain = pipe.factor_screen()
    assert set(plain) == {"ic", "stats", "ir_year", "nrows", "dates_idx", "years", "year0",
                          "features"}
    got = pipe.factor_screen(layers=True)                   # z=True, train
    assert set(got) == set(plain) | set(LAYER_KEYS)
    for k in ("ic", "stats", "ir_year", "nrows", "dates_idx"):
        assert same(got[k], plain[k]), k
    # by hand on the step's buffers
    sp, T, lda, nch = pipe.sp, pipe.T, pipe.lda, pipe.nch

    def by_hand(t0, t1, rows_bits, **kw):
        rb, pb = torch.zeros_like(pipe.zrows), torch.zeros_like(pipe.alldf)
        _lib.run("afm_row_bits", nch, lda, rows_bits, None, None, t0, t1, rb)
        _lib.run("afm_row_bits", nch, lda, pipe.alldf, None, None, t0, t1, pb)
        return afm.screen_grid(pipe.out, kw.pop("cols", pipe.feat), grid.close, pb, rb, A=grid.A,
                               year=years_of(grid.dates), layers=True, **kw)
    hand = by_hand(0, sp.tr1, pipe.zrows, zs=pipe.zs)
    nd = len(got["dates_idx"])
    assert nd > 100 and got["layer_mean"].shape == (nd, pipe.p, 3, 10)
    assert same(got["dates_idx"], hand["dates_idx"])
    for k in LAYER_KEYS:
        assert same(got[k], hand[k].cpu().numpy()), k
    assert got["layer_cnt"].sum(axis=2).max() > 100 and not np.isnan(got["cum_port"]).all()
    # the step's results are untouched
    after = pipe.summary()
    assert before.keys() == after.keys()
    for k in before:
        assert same(np.asarray(before[k]), np.asarray(after[k])), k
    # raw values on the all_df rows with a column subset; another split
    from afm.factors import COL
    raw = pipe.factor_screen(z=False, columns=["RSI_14", "target"], layers=True)
    hand = by_hand(0, sp.tr1, pipe.alldf, cols=np.array([COL["RSI_14"], COL["target"]], np.int32))
    assert raw["layer_mean"].shape[1:] == (2, 3, 10)
    for k in LAYER_KEYS:
        assert same(raw[k], hand[k].cpu().numpy()), k
    val = pipe.factor_screen(split="valid", layers=True)
    hand = by_hand(sp.v0, sp.v1, pipe.zrows, zs=pipe.zs)
    assert sp.v0 <= val["dates_idx"].min() and val["dates_idx"].max() < sp.v1
    assert same(val["dates_idx"], hand["dates_idx"])
    for k in LAYER_KEYS:
        assert same(val[k], hand[k].cpu().numpy()), k
    # one GPU only
    two = Pipeline(grid, PipelineConfig(**SPLIT), EmulatedComm(2, 0))
    with pytest.raises(NotImplementedError):
        two.factor_screen(layers=True)
