"""The rank (Spearman) IC through the public interface: ``AlphaSignalAnalyzer`` with
``corr_method = 'spearman'`` and ``FactorScreen(..., corr_method='spearman')`` against the pandas
statement on a ragged frame, ``screen_grid`` against the single-factor path it batches, and
``Pipeline.factor_screen`` on a stepped pipeline.  Bit for bit, NaN equal to NaN."""
import numpy as np
import pandas as pd
import pytest

import analyzer_ref as R
import rank_ref as K
import screen_ref as S
from helpers import same
from test_sharded import SPLIT

pytestmark = pytest.mark.gpu

NAMES = list("abcde")


def years_of(dates):
    return np.asarray(dates).astype("datetime64[Y]").astype(np.int64) + 1970


@pytest.fixture(scope="module")
def ragged():
    """40 dates over two calendar years, 150 ids, price rows with p = 0.9, factor rows a subset of
    them; 5 columns: 'a' clean, 'b' rounded (ties), 'c' with NaN and inf cells, 'd' constant,
    'e' with +-inf cells and no NaN (a frame the analyzer takes).  The references in pandas on the
    same rows: ``DataFrame.corr`` per date, Spearman and Pearson, and the summary of the former."""
    rng = np.random.default_rng(23)
    T, A = 40, 150
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
    F[4][rng.random((T, A)) < 0.02] = np.inf
    F[4][rng.random((T, A)) < 0.02] = -np.inf
    F[4, 7] = rng.normal(size=A)                           # a date without inf: the fast path
    tt, aa = np.nonzero(inframe)
    df = pd.DataFrame({c: F[j, tt, aa] for j, c in enumerate(NAMES)},
                      index=pd.MultiIndex.from_arrays([dates[tt], ids[aa]]))
    pt, pa = np.nonzero(present)
    price = pd.DataFrame({"close_price": close[pt, pa]},
                         index=pd.MultiIndex.from_arrays([dates[pt], ids[pa]]))
    fr = R.fwd_returns_ref(np.where(present, close, np.nan), present)
    prep = R.prepare_ref(np.where(inframe, 0.0, np.nan), fr)
    didx = [t for t in range(T) if len(prep[t][0])]
    ic = np.stack([K.ic_pandas_wide(F[:, t, prep[t][0]], prep[t][1][1:]) for t in didx])
    pearson = np.stack([S.ic_pandas_wide(F[:, t, prep[t][0]], prep[t][1][1:]) for t in didx])
    yr = years_of(dates)[didx].astype(np.int32)
    y0, ny = int(yr.min()), int(yr.max() - yr.min() + 1)
    stats, ir_year = S.summary_pandas(ic, yr, ny, y0)
    return dict(df=df, price=price, dates=dates[didx], ic=ic, pearson=pearson, yr=yr, y0=y0,
                stats=stats, ir_year=ir_year)


def analyzer(g, col, method=None):
    import afm
    an = afm.AlphaSignalAnalyzer(g["df"][[col]].copy(), col, g["price"].copy())
    if method is not None:
        an.corr_method = method                            # the reference's interface: the attribute
    an.run()
    return an


def expect_ic_ir(g, k, ic):
    """The rows of ic_df / ir_df for column k of the reference ICs ``ic`` [nd][5][3]."""
    want = [(d, R.RETURNS[q], ic[i, k, q]) for i, d in enumerate(g["dates"]) for q in range(3)
            if ic[i, k, q] == ic[i, k, q]]
    _, ir_year = S.summary_pandas(ic[:, k:k + 1], g["yr"], g["ir_year"].shape[0], g["y0"])
    has = [(y, q) for y in range(ir_year.shape[0]) for q in range(3)
           if (~np.isnan(ic[g["yr"] == g["y0"] + y, k, q])).any()]
    return want, [(g["y0"] + y, R.RETURNS[q], ir_year[y, 0, q]) for y, q in has]


@pytest.mark.parametrize("col", ["b", "e"])
def test_analyzer_spearman(ragged, col):
    """``an.corr_method = 'spearman'; an.run()``: ic_df / ir_df are pandas' rank ICs (ties in 'b';
    +-inf cells in 'e': the masked path), every other frame is the Pearson run's, and the default
    run is still the Pearson statement."""
    g, k = ragged, NAMES.index(col)
    sp, pe, default = analyzer(g, col, "spearman"), analyzer(g, col, "pearson"), analyzer(g, col)
    for an, ic in ((sp, g["ic"]), (pe, g["pearson"]), (default, g["pearson"])):
        want, want_ir = expect_ic_ir(g, k, ic)
        assert len(want) > 90
        assert same(an.ic_df["date"].values.astype(np.int64),
                    np.array([w[0] for w in want]).astype("datetime64[ns]").astype(np.int64))
        assert list(an.ic_df["Type"]) == [w[1] for w in want]
        assert same(an.ic_df["IC"].values, np.array([w[2] for w in want]))
        assert list(an.ir_df["year"]) == [w[0] for w in want_ir]
        assert list(an.ir_df["Type"]) == [w[1] for w in want_ir]
        assert same(an.ir_df["IR"].values, np.array([w[2] for w in want_ir]))
    assert default.corr_method == "pearson"
    assert not same(sp.ic_df["IC"].values, pe.ic_df["IC"].values)
    assert same(sp._res["ic_pearson"].cpu().numpy(), pe._res["ic"].cpu().numpy())
    assert same(sp.factor_df.to_numpy(np.float64), pe.factor_df.to_numpy(np.float64))
    for rt in R.RETURNS:
        assert sp.layered_ret_dfs[rt].equals(pe.layered_ret_dfs[rt])
        assert sp.ls_ret_dfs[rt].equals(pe.ls_ret_dfs[rt])
    assert sp.port_ret_df.equals(pe.port_ret_df) and sp.port_df.equals(pe.port_df)


def test_analyzer_rejects_other_methods(ragged):
    import afm
    for method, exc in (("kendall", NotImplementedError), ("rank", ValueError)):
        an = afm.AlphaSignalAnalyzer(ragged["df"][["a"]].copy(), "a", ragged["price"].copy())
        an.corr_method = method
        with pytest.raises(exc):
            an.run()


def test_factor_screen_spearman(ragged):
    """FactorScreen(..., corr_method='spearman'): ic_df of every column (NaN / inf cells skipped
    for their own column only) is pandas', summary / ir_df are the pandas summary of the rank ICs,
    and a NaN-free column's rows are the per-column analyzer's."""
    import afm
    g = ragged
    fs = afm.FactorScreen(g["df"].copy(), g["price"].copy(), corr_method="spearman").run()
    types, ic = list(R.RETURNS), g["ic"]
    assert ic.shape[0] > 30 and np.isnan(ic[:, 3]).all() and not np.isnan(ic[:, 2]).all()
    want = [(d, NAMES[k], types[q], ic[i, k, q]) for i, d in enumerate(g["dates"])
            for k in range(5) for q in range(3) if ic[i, k, q] == ic[i, k, q]]
    assert same(fs.ic_df["date"].values.astype(np.int64),
                np.array([w[0] for w in want]).astype("datetime64[ns]").astype(np.int64))
    assert list(fs.ic_df["factor"]) == [w[1] for w in want]
    assert list(fs.ic_df["Type"]) == [w[2] for w in want]
    assert same(fs.ic_df["IC"].values, np.array([w[3] for w in want]))
    has = [(y, k, q) for y in range(g["ir_year"].shape[0]) for k in range(5) for q in range(3)
           if (~np.isnan(ic[g["yr"] == g["y0"] + y, k, q])).any()]
    assert list(fs.ir_df["year"]) == [g["y0"] + y for y, _, _ in has]
    assert list(fs.ir_df["factor"]) == [NAMES[k] for _, k, _ in has]
    assert same(fs.ir_df["IR"].values, np.array([g["ir_year"][h] for h in has]))
    st = g["stats"].reshape(15, 5)
    key = np.abs(st[:, 3])
    order = sorted(range(15), key=lambda i: (np.isnan(key[i]), -key[i] if key[i] == key[i] else 0, i))
    assert list(fs.summary["factor"]) == [NAMES[i // 3] for i in order]
    assert list(fs.summary["Type"]) == [types[i % 3] for i in order]
    assert same(fs.summary[["n", "mean", "std", "IR", "t"]].to_numpy(np.float64), st[order])
    # a column without NaN against the single-factor analyzer
    for col in ("b", "e"):
        an = analyzer(g, col, "spearman")
        mine = fs.ic_df[fs.ic_df["factor"] == col]
        assert len(mine) == len(an.ic_df) > 90
        assert same(mine["date"].values.astype(np.int64), an.ic_df["date"].values.astype(np.int64))
        assert list(mine["Type"]) == list(an.ic_df["Type"])
        assert same(mine["IC"].values, an.ic_df["IC"].values)
        mir = fs.ir_df[fs.ir_df["factor"] == col]
        assert list(mir["year"]) == list(an.ir_df["year"])
        assert same(mir["IR"].values, an.ir_df["IR"].values)
    # the default is still the Pearson screen
    pe = afm.FactorScreen(g["df"].copy(), g["price"].copy()).run()
    pwant = np.array([g["pearson"][i, k, q] for i in range(len(g["dates"])) for k in range(5)
                      for q in range(3) if g["pearson"][i, k, q] == g["pearson"][i, k, q]])
    assert pe.corr_method == "pearson" and same(pe.ic_df["IC"].values, pwant)
    with pytest.raises(NotImplementedError):
        afm.FactorScreen(g["df"], g["price"], corr_method="kendall")
    with pytest.raises(ValueError):
        afm.FactorScreen(g["df"], g["price"], corr_method="rank")


def test_screen_grid_equals_the_single_factor_path():
    """200 assets x 300 dates, 8 raw panel columns on the panel's NaN-free rows: for each column
    ``evaluate_grid(corr_method='spearman')``'s IC and per-year IR are the screen's, bit for bit;
    its ``ic_pearson`` is the Pearson screen's column."""
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
    scr = afm.screen_grid(out, cols, grid.close, grid.vbits, nanfree, A=grid.A, year=year,
                          corr_method="spearman")
    ic, iry = scr["ic"].cpu().numpy(), scr["ir_year"].cpu().numpy()
    pearson = afm.screen_grid(out, cols, grid.close, grid.vbits, nanfree, A=grid.A,
                              year=year)["ic"].cpu().numpy()
    assert ic.shape[0] > 200 and not np.isnan(ic).all() and not same(ic, pearson)
    rowm = afm.unpack_bits(nanfree, grid.T)
    for k, c in enumerate(cols):
        sig = torch.where(rowm, out[c], torch.full_like(out[c], float("nan")))
        one = evaluate_grid(sig, grid.close, grid.vbits, A=grid.A, year=year,
                            corr_method="spearman")
        assert same(one["dates_idx"], scr["dates_idx"])
        assert same(one["ic"].cpu().numpy(), ic[:, k, :]), names[k]
        assert same(one["ir"].cpu().numpy(), iry[:, k, :]), names[k]
        assert same(one["ic_pearson"].cpu().numpy(), pearson[:, k, :]), names[k]
    # one date against pandas itself, on the rows the screen reports
    i = ic.shape[0] // 2
    t = int(scr["dates_idx"][i])
    n = int(scr["nrows"][t].item())
    idx = scr["rows_idx"][t, :n].long()
    rets = evaluate_grid(sig, grid.close, grid.vbits, A=grid.A)["rows"][1:, t, :n].cpu().numpy()
    F = out[torch.from_numpy(cols).long().to(out.device)][:, t, idx].cpu().numpy()
    assert same(ic[i], K.ic_pandas_wide(F, rets))


def test_pipeline_factor_screen_spearman():
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
    got = pipe.factor_screen(corr_method="spearman")        # z=True, train
    sp, lda, nch = pipe.sp, pipe.lda, pipe.nch
    rb, pb = torch.zeros_like(pipe.zrows), torch.zeros_like(pipe.alldf)
    _lib.run("afm_row_bits", nch, lda, pipe.zrows, None, None, 0, sp.tr1, rb)
    _lib.run("afm_row_bits", nch, lda, pipe.alldf, None, None, 0, sp.tr1, pb)
    hand = afm.screen_grid(pipe.out, pipe.feat, grid.close, pb, rb, A=grid.A, zs=pipe.zs,
                           year=years_of(grid.dates), corr_method="spearman")
    assert got["features"] == pipe.features and got["ic"].shape[1:] == (pipe.p, 3)
    assert same(got["dates_idx"], hand["dates_idx"]) and len(got["dates_idx"]) > 100
    for k in ("ic", "stats", "ir_year"):
        assert same(got[k], hand[k].cpu().numpy()), k
    assert (~np.isnan(got["ic"])).sum() > got["ic"].size // 2
    pearson = pipe.factor_screen()
    assert same(pearson["dates_idx"], got["dates_idx"]) and not same(pearson["ic"], got["ic"])
    raw = pipe.factor_screen(z=False, columns=["RSI_14", "target"], corr_method="spearman")
    assert raw["ic"].shape[1:] == (2, 3) and not np.isnan(raw["ic"]).all()
    assert not same(raw["ic"], pipe.factor_screen(z=False, columns=["RSI_14", "target"])["ic"])
    # the step's results are untouched
    after = pipe.summary()
    assert before.keys() == after.keys()
    for k in before:
        assert same(np.asarray(before[k]), np.asarray(after[k])), k
    with pytest.raises(NotImplementedError):
        pipe.factor_screen(corr_method="kendall")
    with pytest.raises(ValueError, match="corr_method"):
        pipe.factor_screen(corr_method="rank")
    two = Pipeline(grid, PipelineConfig(**SPLIT), EmulatedComm(2, 0))
    with pytest.raises(NotImplementedError):
        two.factor_screen(corr_method="spearman")
