"""The cross-factor correlation of the factor screen end to end: ``screen_grid(xcorr=True)`` and
``FactorScreen(xcorr=True)`` against ``groupby(date).corr()`` of a ragged frame, ``select()``
against ``select_factors``, and ``Pipeline.factor_screen(xcorr=True)`` on a stepped pipeline against
the extended-precision reference (tests/xcorr_ref.py) on the panel copied to the host.  Values
within 32 max(n, 64) 2^-53 of the date's row count, NaN patterns equal; what the screen gave
before is unchanged bit for bit."""
import numpy as np
import pandas as pd
import pytest

import analyzer_ref as R
import xcorr_ref as X
from helpers import same
from test_sharded import SPLIT

pytestmark = pytest.mark.gpu

NAMES = list("abcde")
TODAY_KEYS = {"ic", "stats", "ir_year", "nrows", "rows_idx", "dates_idx", "years", "year0"}


def years_of(dates):
    return np.asarray(dates).astype("datetime64[Y]").astype(np.int64) + 1970


@pytest.fixture(scope="module")
def ragged():
    """The frame tests/test_screen_layers_gpu.py builds (the same generator and seed): 40 dates, 90
    ids, price rows with p = 0.9, factor rows a subset; 'a' clean, 'b' rounded, 'c' with NaN and inf
    cells, 'd' constant, 'e' = -a.  And per evaluated date the pandas correlation matrix of the
    columns over the screen's rows (the frame's rows that have forward returns)."""
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
    rowsel = np.zeros((T, A), dtype=bool)
    for t in didx:
        rowsel[t, prep[t][0]] = True
    st, sa = np.nonzero(rowsel)
    rows_df = pd.DataFrame({c: F[j, st, sa] for j, c in enumerate(NAMES)},
                           index=pd.MultiIndex.from_arrays([dates[st], ids[sa]],
                                                           names=["date", "id"]))
    with np.errstate(all="ignore"):
        gc = rows_df.replace([np.inf, -np.inf], np.nan).groupby(level="date").corr()
    want = np.stack([gc.loc[pd.Timestamp(dates[t])].loc[NAMES, NAMES].to_numpy() for t in didx])
    counts = np.array([len(prep[t][0]) for t in didx])
    return dict(df=df, price=price, dates=dates[didx], want=want, counts=counts, F=F, T=T, A=A,
                present=present, inframe=inframe, close=close, all_dates=dates)


def within(got, want, counts, what):
    assert got.shape == want.shape, what
    worst = 0.0
    for i, n in enumerate(counts):
        assert (np.isnan(got[i]) == np.isnan(want[i])).all(), (what, i, int(n))
        if not np.isnan(want[i]).all():
            err = float(np.nanmax(np.abs(got[i] - want[i])))
            worst = max(worst, err / X.tolerance(n))
    print(f"xcorr error {what}: largest |xc - ref| / bound = {worst:.3e}")
    assert worst <= 1.0, what


def test_screen_grid_xcorr_equals_groupby_corr(ragged):
    import torch
    import afm
    g = ragged
    T, A = g["T"], g["A"]
    lda = 128
    dev = torch.device("cuda", 0)
    base = torch.full((5, T, lda), float("nan"), dtype=torch.float64, device=dev)
    base[:, :, :A] = torch.from_numpy(g["F"]).to(dev)
    close = torch.full((T, lda), float("nan"), dtype=torch.float64, device=dev)
    close[:, :A] = torch.from_numpy(np.where(g["present"], g["close"], np.nan)).to(dev)
    pm = torch.zeros((T, lda), dtype=torch.bool, device=dev)
    pm[:, :A] = torch.from_numpy(g["present"]).to(dev)
    rm = torch.zeros((T, lda), dtype=torch.bool, device=dev)
    rm[:, :A] = torch.from_numpy(g["inframe"]).to(dev)
    args = (base, np.arange(5), close, afm.pack_bits(pm), afm.pack_bits(rm))
    year = years_of(g["all_dates"])
    plain = afm.screen_grid(*args, A=A, year=year)
    assert set(plain) == TODAY_KEYS
    bufs = {}
    scr = afm.screen_grid(*args, A=A, year=year, xcorr=True, bufs=bufs)
    assert set(scr) == TODAY_KEYS | {"xcorr", "xcorr_stats"}
    assert bufs["xcorr"] is scr["xcorr"] and bufs["xcorr_stats"] is scr["xcorr_stats"]
    for k in ("ic", "stats", "ir_year", "nrows"):
        assert same(scr[k].cpu().numpy(), plain[k].cpu().numpy()), k
    nr, ri, rj = plain["nrows"].cpu().numpy(), scr["rows_idx"].cpu().numpy(), \
        plain["rows_idx"].cpu().numpy()
    assert all(same(ri[t, :nr[t]], rj[t, :nr[t]]) for t in range(T))     # the rows in use
    assert same(scr["dates_idx"], plain["dates_idx"])
    xc = scr["xcorr"].cpu().numpy()
    assert xc.shape == (len(g["dates"]), 5, 5)
    within(xc, g["want"], g["counts"], "screen_grid")
    assert np.isnan(xc[:, 3, :]).all() and np.isnan(xc[:, :, 3]).all()      # 'd' constant
    assert (xc[:, 0, 4] >= -1.0).all() and np.abs(xc[:, 0, 4] + 1.0).max() < 1e-13   # 'e' = -a
    assert same(scr["xcorr_stats"].cpu().numpy(), X.summary_ref(xc))
    # the factor-to-factor correlation is Pearson whatever the IC's method is
    rank = afm.screen_grid(*args, A=A, year=year, xcorr=True, corr_method="spearman")
    assert same(rank["xcorr"].cpu().numpy(), xc)
    assert not same(rank["ic"].cpu().numpy(), scr["ic"].cpu().numpy())
    lay = afm.screen_grid(*args, A=A, year=year, xcorr=True, layers=True)
    assert same(lay["xcorr"].cpu().numpy(), xc) and "layer_mean" in lay


def test_factor_screen_frames_and_select(ragged):
    import afm
    from afm.screen import select_factors
    g = ragged
    fs = afm.FactorScreen(g["df"].copy(), g["price"].copy(), xcorr=True).run()
    plain = afm.FactorScreen(g["df"].copy(), g["price"].copy()).run()
    assert plain.ic_df.equals(fs.ic_df) and plain.summary.equals(fs.summary)
    assert plain.ir_df.equals(fs.ir_df) and not hasattr(plain, "factor_corr")
    with pytest.raises(ValueError):
        plain.select()
    want = X.summary_ref(fs._res["xcorr"].cpu().numpy())
    within(fs._res["xcorr"].cpu().numpy(), g["want"], g["counts"], "FactorScreen")
    for frame, j in ((fs.factor_corr_n, 0), (fs.factor_corr, 1), (fs.factor_corr_abs, 2)):
        assert list(frame.index) == NAMES and list(frame.columns) == NAMES
        assert same(frame.to_numpy().astype(np.float64), want[:, :, j])
    assert fs.factor_corr_n.to_numpy().dtype == np.int64
    nd = len(g["dates"])
    assert fs.factor_corr_n.loc["a", "b"] == nd and fs.factor_corr_n.loc["a", "d"] == 0
    assert np.isnan(fs.factor_corr.loc["d", "d"]) and fs.factor_corr.loc["a", "a"] == 1.0
    ok = ~np.isnan(g["want"]).all(axis=0)
    ref_mean = np.where(ok, np.nansum(g["want"], axis=0) / np.maximum(
        (~np.isnan(g["want"])).sum(axis=0), 1), np.nan)
    assert np.abs(fs.factor_corr.to_numpy()[ok] - ref_mean[ok]).max() <= X.tolerance(90)
    # redundant_pairs: j < k with n > 0, by mean_abs descending, ties in column order
    rp = fs.redundant_pairs
    assert list(rp.columns) == ["factor_a", "factor_b", "mean", "mean_abs", "n"]
    rows = [(a, b, want[i, j, 1], want[i, j, 2], int(want[i, j, 0]))
            for i, a in enumerate(NAMES) for j, b in enumerate(NAMES) if i < j and want[i, j, 0] > 0]
    order = sorted(range(len(rows)), key=lambda i: (-rows[i][3], i))
    assert len(rp) == len(rows) == 6                        # the pairs without 'd'
    assert list(zip(rp["factor_a"], rp["factor_b"])) == [rows[i][:2] for i in order]
    assert same(rp["mean"].values, np.array([rows[i][2] for i in order]))
    assert same(rp["mean_abs"].values, np.array([rows[i][3] for i in order]))
    assert list(rp["n"]) == [rows[i][4] for i in order] and rp["n"].dtype == np.int64
    assert (rp["factor_a"].iloc[0], rp["factor_b"].iloc[0]) == ("a", "e")
    # select() is select_factors on the frames with the whole-sample IR of the return type
    for rt in fs.return_type:
        s = fs.summary[fs.summary["Type"] == rt].set_index("factor").loc[NAMES, "IR"].to_numpy()
        for mc, k in ((0.7, None), (0.05, None), (1.0, 2), (0.7, 1)):
            assert fs.select(mc, k, rt) == select_factors(NAMES, s, fs.factor_corr_abs.to_numpy(),
                                                          mc, k)
    sel = fs.select()
    assert "d" not in sel and not {"a", "e"} <= set(sel) and 2 <= len(sel) <= 3
    sub = afm.FactorScreen(g["df"].copy(), g["price"].copy(), columns=["e", "b"], xcorr=True).run()
    assert list(sub.factor_corr.index) == ["e", "b"]
    assert sub.factor_corr.loc["e", "b"] == -fs.factor_corr.loc["a", "b"] or \
        abs(sub.factor_corr.loc["e", "b"] + fs.factor_corr.loc["a", "b"]) < 1e-13


def test_pipeline_factor_screen_xcorr():
    import torch
    import afm
    from afm import _lib
    from afm.factors import COL
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.screen import select_factors
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
    got = pipe.factor_screen(xcorr=True)                    # z=True, train, every feature
    assert set(got) == set(plain) | {"xcorr_stats", "xcorr_dev"}
    assert got["features"] == plain["features"]
    for k in set(plain) - {"features"}:                     # what the screen gave before: unchanged
        assert same(np.asarray(got[k]), np.asarray(plain[k])), k
    p, nd = pipe.p, len(got["dates_idx"])
    assert nd > 100 and got["xcorr_stats"].shape == (p, p, 3)
    assert isinstance(got["xcorr_stats"], np.ndarray) and got["xcorr_dev"].is_cuda
    assert tuple(got["xcorr_dev"].shape) == (nd, p, p)
    xc = got["xcorr_dev"].cpu().numpy()
    assert same(got["xcorr_stats"], X.summary_ref(xc))
    assert same(xc, xc.transpose(0, 2, 1))
    # the reference on the panel copied to the host: the rows of the screen from a call by hand
    sp, T, lda, nch = pipe.sp, pipe.T, pipe.lda, pipe.nch

    def rows_of(t0, t1, rows_bits):
        rb, pb = torch.zeros_like(pipe.zrows), torch.zeros_like(pipe.alldf)
        _lib.run("afm_row_bits", nch, lda, rows_bits, None, None, t0, t1, rb)
        _lib.run("afm_row_bits", nch, lda, pipe.alldf, None, None, t0, t1, pb)
        r = afm.screen_grid(pipe.out, pipe.feat[:1], grid.close, pb, rb, A=grid.A)
        return r["rows_idx"].cpu().numpy(), r["nrows"].cpu().numpy()
    out = pipe.out.cpu().numpy()
    zs = pipe.zs.cpu().numpy()
    ridx, nrows = rows_of(0, sp.tr1, pipe.zrows)
    assert same(nrows, got["nrows"])
    feat = [COL[n] for n in got["features"]]
    some = np.linspace(0, nd - 1, 12).astype(int)            # every feature on a dozen dates
    ref = np.stack([X.corr_ref(X.date_values(out, ridx, nrows, got["dates_idx"][i], feat, zs,
                                             np.arange(p))) for i in some])
    within(xc[some], ref, nrows[got["dates_idx"][some]], "pipeline z, all features")
    # a column subset on every date: the stats against the reference's
    names = [got["features"][i] for i in (0, 5, 11, 17, 23, 40, 41, p - 1)]
    for z, bits in ((True, pipe.zrows), (False, pipe.alldf)):
        r = pipe.factor_screen(z=z, columns=names, xcorr=True)
        if not z:
            ridx, nrows = rows_of(0, sp.tr1, bits)
        cols = [COL[n] for n in names]
        zc = [got["features"].index(n) for n in names]
        ref = np.stack([X.corr_ref(X.date_values(out, ridx, nrows, t, cols, zs if z else None, zc))
                        for t in r["dates_idx"]])
        counts = nrows[r["dates_idx"]]
        sub = r["xcorr_dev"].cpu().numpy()
        within(sub, ref, counts, f"pipeline z={z}, 8 columns")
        st, want = r["xcorr_stats"], X.summary_ref(ref)
        assert same(st[:, :, 0], want[:, :, 0]) and st.shape == (8, 8, 3)
        ok = want[:, :, 0] > 0
        assert np.abs(st[ok][:, 1:] - want[ok][:, 1:]).max() <= X.tolerance(counts.max())
        if z:
            i = [got["features"].index(n) for n in names]
            assert same(sub, xc[:, i][:, :, i])              # the same entries as among all features
    # the step's results are untouched
    after = pipe.summary()
    for k in before:
        assert same(np.asarray(before[k]), np.asarray(after[k])), k
    # screen -> select -> a Fama-MacBeth design that steps
    sel = select_factors(got["features"], got["stats"][:, 0, 3], got["xcorr_stats"][:, :, 2],
                         max_corr=0.7, k=12)
    assert 2 <= len(sel) <= 12 and len(set(sel)) == len(sel)
    idx = [got["features"].index(n) for n in sel]
    pair = got["xcorr_stats"][np.ix_(idx, idx)][:, :, 2]
    assert (pair[~np.eye(len(sel), dtype=bool)] <= 0.7).all()
    pipe2 = Pipeline(grid, PipelineConfig(fm_features=tuple(sel), **SPLIT))
    pipe2.step()
    torch.cuda.synchronize()
    s2 = pipe2.summary()
    assert pipe2.pf == len(sel) and np.isfinite(s2["final_value"])
    assert np.isfinite(s2["fm_mean"]).all()
    # one GPU only
    two = Pipeline(grid, PipelineConfig(**SPLIT), EmulatedComm(2, 0))
    with pytest.raises(NotImplementedError):
        two.factor_screen(xcorr=True)
