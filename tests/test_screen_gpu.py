"""Factor screening end to end: ``screen_grid`` against the single-factor path it batches
(``evaluate_grid``, whose kernels have bit-exact reference goldens), ``FactorScreen`` against the
pandas statement on a ragged frame, and ``Pipeline.factor_screen`` on a stepped pipeline.  Bit for
bit, NaN equal to NaN."""
import numpy as np
import pandas as pd
import pytest

import analyzer_ref as R
import screen_ref as S
from helpers import same
from test_sharded import SPLIT

pytestmark = pytest.mark.gpu


def years_of(dates):
    return np.asarray(dates).astype("datetime64[Y]").astype(np.int64) + 1970


# ---- screen_grid == K calls of evaluate_grid ----------------------------------------------------------
def test_screen_grid_equals_the_single_factor_path():
    """200 assets x 300 dates, 8 raw panel columns on the panel's NaN-free rows: for each column
    the analyzer's own IC and per-year IR (sig = the column on the row set, NaN elsewhere) are
    the screen's, bit for bit -- same rows, same demeans, same recurrence."""
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
    scr = afm.screen_grid(out, cols, grid.close, grid.vbits, nanfree, A=grid.A, year=year)
    rowm = afm.unpack_bits(nanfree, grid.T)
    ic, iry = scr["ic"].cpu().numpy(), scr["ir_year"].cpu().numpy()
    assert ic.shape[0] > 200 and not np.isnan(ic).all()
    for k, c in enumerate(cols):
        assert not torch.isnan(out[c][rowm]).any()
        sig = torch.where(rowm, out[c], torch.full_like(out[c], float("nan")))
        one = evaluate_grid(sig, grid.close, grid.vbits, A=grid.A, year=year)
        assert same(one["dates_idx"], scr["dates_idx"])
        assert same(one["nrows"].cpu().numpy(), scr["nrows"].cpu().numpy())
        assert same(one["ic"].cpu().numpy(), ic[:, k, :]), names[k]
        assert one["year0"] == scr["year0"]
        assert same(one["ir"].cpu().numpy(), iry[:, k, :]), names[k]


# ---- FactorScreen on a ragged frame ----------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    """40 dates over two calendar years, 90 ids, price rows with p = 0.9, factor rows a subset of
    them; 5 columns: 'a' clean, 'b' rounded (ties), 'c' with NaN and inf cells, 'd' constant,
    'e' = -a (|IR| ties with 'a')."""
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
    df = pd.DataFrame({c: F[j, tt, aa] for j, c in enumerate("abcde")},
                      index=pd.MultiIndex.from_arrays([dates[tt], ids[aa]]))
    pt, pa = np.nonzero(present)
    price = pd.DataFrame({"close_price": close[pt, pa]},
                         index=pd.MultiIndex.from_arrays([dates[pt], ids[pa]]))
    # the pandas / numpy statement on the same rows (tests/analyzer_ref.py, tests/screen_ref.py)
    fr = R.fwd_returns_ref(np.where(present, close, np.nan), present)
    prep = R.prepare_ref(np.where(inframe, 0.0, np.nan), fr)
    didx = [t for t in range(T) if len(prep[t][0])]
    ic = np.stack([S.ic_pandas_wide(F[:, t, prep[t][0]], prep[t][1][1:]) for t in didx])
    yr = years_of(dates)[didx].astype(np.int32)
    y0, ny = int(yr.min()), int(yr.max() - yr.min() + 1)
    stats, ir_year = S.summary_pandas(ic, yr, ny, y0)
    return dict(df=df, price=price, dates=dates[didx], ic=ic, yr=yr, y0=y0, stats=stats,
                ir_year=ir_year)


def test_factor_screen_frames(ragged):
    import afm
    g = ragged
    fs = afm.FactorScreen(g["df"].copy(), g["price"].copy()).run()
    names, types = list("abcde"), list(R.RETURNS)
    ic = g["ic"]
    assert ic.shape[0] > 30 and np.isnan(ic[:, 3]).all() and not np.isnan(ic[:, 2]).all()
    # ic_df: (date, factor in column order, Type), NaN ICs dropped
    want = [(d, names[k], types[q], ic[i, k, q]) for i, d in enumerate(g["dates"])
            for k in range(5) for q in range(3) if ic[i, k, q] == ic[i, k, q]]
    assert list(fs.ic_df.columns) == ["date", "factor", "Type", "IC"]
    assert same(fs.ic_df["date"].values.astype(np.int64),
                np.array([w[0] for w in want]).astype("datetime64[ns]").astype(np.int64))
    assert list(fs.ic_df["factor"]) == [w[1] for w in want]
    assert list(fs.ic_df["Type"]) == [w[2] for w in want]
    assert same(fs.ic_df["IC"].values, np.array([w[3] for w in want]))
    # ir_df: a row per (year, factor, Type) that has an IC
    has = [(y, k, q) for y in range(g["ir_year"].shape[0]) for k in range(5) for q in range(3)
           if (~np.isnan(ic[g["yr"] == g["y0"] + y, k, q])).any()]
    assert list(fs.ir_df.columns) == ["year", "factor", "Type", "IR"]
    assert list(fs.ir_df["year"]) == [g["y0"] + y for y, _, _ in has]
    assert list(fs.ir_df["factor"]) == [names[k] for _, k, _ in has]
    assert list(fs.ir_df["Type"]) == [types[q] for _, _, q in has]
    assert same(fs.ir_df["IR"].values, np.array([g["ir_year"][h] for h in has]))
    # summary: |IR| descending, ties in column order ('e' = -'a' right after 'a'), NaN last
    st = g["stats"].reshape(15, 5)
    key = np.abs(st[:, 3])
    order = sorted(range(15), key=lambda i: (np.isnan(key[i]), -key[i] if key[i] == key[i] else 0, i))
    assert list(fs.summary.columns) == ["factor", "Type", "n", "mean", "std", "IR", "t"]
    assert list(fs.summary["factor"]) == [names[i // 3] for i in order]
    assert list(fs.summary["Type"]) == [types[i % 3] for i in order]
    assert same(fs.summary[["n", "mean", "std", "IR", "t"]].to_numpy(np.float64), st[order])
    assert list(fs.summary["factor"][-3:]) == ["d"] * 3
    ia = [i for i, f in enumerate(fs.summary["factor"]) if f == "a"]
    assert all(fs.summary["factor"][i + 1] == "e" for i in ia)


def test_factor_screen_column_equals_the_analyzer(ragged):
    """A column without NaN: the rows of ic_df / ir_df are those of the single-factor analyzer."""
    import afm
    g = ragged
    fs = afm.FactorScreen(g["df"].copy(), g["price"].copy(), columns=["b", "a"]).run()
    an = afm.AlphaSignalAnalyzer(g["df"][["b"]].copy(), "b", g["price"].copy())
    an.run()
    mine = fs.ic_df[fs.ic_df["factor"] == "b"]
    assert len(mine) == len(an.ic_df) > 90
    assert same(mine["date"].values.astype(np.int64), an.ic_df["date"].values.astype(np.int64))
    assert list(mine["Type"]) == list(an.ic_df["Type"])
    assert same(mine["IC"].values, an.ic_df["IC"].values)
    mir = fs.ir_df[fs.ir_df["factor"] == "b"]
    assert list(mir["year"]) == list(an.ir_df["year"]) and list(mir["Type"]) == list(an.ir_df["Type"])
    assert same(mir["IR"].values, an.ir_df["IR"].values)


# ---- Pipeline.factor_screen --------------------------------------------------------------------------
def test_pipeline_factor_screen():
    import torch
    import afm
    from afm import _lib
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.sharded import EmulatedComm
    from afm.synthetic import make_panel
    torch.cuda.set_device(0)
    grid = afm.PanelGrid.from_panel(make_panel(300, 700, seed=11, tradable_p=0.9))
    pipe = Pipeline(grid, PipelineConfig(**SPLIT))
    with pytest.raises(ValueError, match="step"):
        pipe.factor_screen()
    pipe.step()
    torch.cuda.synchronize()
    before = pipe.summary()
    got = pipe.factor_screen()                              # z=True, train
    # by hand on the step's buffers
    sp, T, lda, nch = pipe.sp, pipe.T, pipe.lda, pipe.nch
    rb, pb = torch.zeros_like(pipe.zrows), torch.zeros_like(pipe.alldf)
    _lib.run("afm_row_bits", nch, lda, pipe.zrows, None, None, 0, sp.tr1, rb)
    _lib.run("afm_row_bits", nch, lda, pipe.alldf, None, None, 0, sp.tr1, pb)
    hand = afm.screen_grid(pipe.out, pipe.feat, grid.close, pb, rb, A=grid.A, zs=pipe.zs,
                           year=years_of(grid.dates))
    assert got["features"] == pipe.features and got["ic"].shape[1:] == (pipe.p, 3)
    assert same(got["dates_idx"], hand["dates_idx"]) and len(got["dates_idx"]) > 100
    assert got["dates_idx"].max() < sp.tr1
    for k in ("ic", "stats", "ir_year"):
        assert same(got[k], hand[k].cpu().numpy()), k
    assert same(got["nrows"], hand["nrows"].cpu().numpy())
    assert (~np.isnan(got["ic"])).sum() > got["ic"].size // 2
    # the step's results are untouched
    after = pipe.summary()
    assert before.keys() == after.keys()
    for k in before:
        assert same(np.asarray(before[k]), np.asarray(after[k])), k
    # the other modes run: raw values on the all_df rows, another split, a column subset
    raw = pipe.factor_screen(z=False, columns=["RSI_14", "target"])
    assert raw["ic"].shape[1:] == (2, 3) and not np.isnan(raw["ic"]).all()
    val = pipe.factor_screen(split="valid")
    assert sp.v0 <= val["dates_idx"].min() and val["dates_idx"].max() < sp.v1
    assert not np.isnan(val["stats"][:, :, 1]).all()
    with pytest.raises(ValueError, match="split"):
        pipe.factor_screen(split="all")
    # one GPU only
    two = Pipeline(grid, PipelineConfig(**SPLIT), EmulatedComm(2, 0))
    with pytest.raises(NotImplementedError):
        two.factor_screen()
