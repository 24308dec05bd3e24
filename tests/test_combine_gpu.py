"""The factor combination end to end on a ragged frame (60 dates x 40 ids x 6 columns):
``screen_grid(combine=...)`` against ``ic_weights`` / ``combine_grid`` / a one-column screen on its
own buffers, ``FactorScreen(combine=...)`` and ``combine_factors`` against the restatements of
tests/combine_ref.py, ``combine=None`` against a plain run, and ``Pipeline.factor_screen(combine=
...)`` against ``screen_grid`` called by hand.  Bit for bit unless said otherwise."""
import numpy as np
import pandas as pd
import pytest

import combine_ref as R
from helpers import same
from test_sharded import SPLIT

pytestmark = pytest.mark.gpu

NAMES = list("abcdef")


@pytest.fixture(scope="module")
def ragged():
    """60 dates, 40 ids, price rows with p = 0.9, factor rows a subset; 'a' and 'b' carry some of
    the next return, 'c' has NaN and inf cells, 'd' is constant, 'e' noise, 'f' = -'a' + noise."""
    rng = np.random.default_rng(31)
    T, A = 60, 40
    dates = np.asarray(np.busday_offset(np.datetime64("2020-02-03"), np.arange(T), roll="forward"),
                       dtype="datetime64[ns]")
    ids = 300 + 3 * np.arange(A)
    present = rng.random((T, A)) < 0.9
    ret = rng.normal(0, 0.02, (T, A))
    close = 30 * np.exp(np.cumsum(ret, axis=0))
    nxt = np.vstack([ret[1:], np.zeros((1, A))])
    inframe = present & (rng.random((T, A)) < 0.85)
    F = rng.normal(size=(6, T, A))
    F[0] += 40 * nxt
    F[1] = np.round(F[1] + 25 * nxt, 1)
    F[2][rng.random((T, A)) < 0.1] = np.nan
    F[2][rng.random((T, A)) < 0.03] = np.inf
    F[3] = 1.5
    F[5] = -F[0] + 0.5 * F[5]
    tt, aa = np.nonzero(inframe)
    idx = pd.MultiIndex.from_arrays([dates[tt], ids[aa]], names=["date", "id"])
    df = pd.DataFrame({c: F[j, tt, aa] for j, c in enumerate(NAMES)}, index=idx)
    pt, pa = np.nonzero(present)
    price = pd.DataFrame({"close_price": close[pt, pa]},
                         index=pd.MultiIndex.from_arrays([dates[pt], ids[pa]]))
    sector = pd.Series(rng.integers(0, 4, size=A)[aa], index=idx, name="group_id")
    return dict(df=df, price=price, groups=sector)


@pytest.fixture(scope="module")
def grids(ragged):
    """The frame and its prices as FactorScreen lays them out on the device."""
    import torch
    from afm import pack_bits
    df, price = ragged["df"], ragged["price"]
    dev = torch.device("cuda", 0)
    sd = df.index.get_level_values(0).to_numpy().astype("datetime64[ns]")
    si = df.index.get_level_values(1).to_numpy().astype(np.int64)
    pd_ = price.index.get_level_values(0).to_numpy().astype("datetime64[ns]")
    pi_ = price.index.get_level_values(1).to_numpy().astype(np.int64)
    dates, ids = np.unique(np.concatenate([sd, pd_])), np.unique(np.concatenate([si, pi_]))
    T, A, K = len(dates), len(ids), len(NAMES)
    lda = (A + 63) // 64 * 64
    st, sa = np.searchsorted(dates, sd), np.searchsorted(ids, si)
    base = np.full((K, T, lda), np.nan)
    base[:, st, sa] = df[NAMES].to_numpy(np.float64).T
    rm = np.zeros((T, lda), dtype=bool)
    rm[st, sa] = True
    pt, pa = np.searchsorted(dates, pd_), np.searchsorted(ids, pi_)
    close = np.full((T, lda), np.nan)
    close[pt, pa] = price["close_price"].to_numpy(np.float64)
    pm = np.zeros((T, lda), dtype=bool)
    pm[pt, pa] = True
    groups = np.full((T, lda), -1, dtype=np.int32)
    groups[st, sa] = ragged["groups"].to_numpy().astype(np.int32)
    to = lambda x: torch.from_numpy(x).to(dev)                             # noqa: E731
    return dict(base=to(base), close=to(close), price_bits=pack_bits(to(pm)),
                row_bits=pack_bits(to(rm)), groups=to(groups), A=A, T=T, lda=lda, K=K,
                host_base=base, st=st, sa=sa, dates=dates, ids=ids)


def screen(g, **kw):
    import afm
    return afm.screen_grid(g["base"], np.arange(g["K"]), g["close"], g["price_bits"],
                           g["row_bits"], A=g["A"], **kw)


def spec_of(method="icir", **kw):
    from afm import ICWeights
    return ICWeights(method, **{"window": 10, "min_periods": 3, **kw})


@pytest.mark.parametrize("method", ["equal", "ic", "icir", "maxir"])
def test_screen_grid_combine_on_its_own_buffers(grids, method):
    import afm
    g = grids
    spec = spec_of(method)
    r = screen(g, combine=spec)
    nd = len(r["dates_idx"])
    assert nd > 40 and r["weights"].shape == (nd, g["K"]) and r["weights_info"].shape == (nd, 3)
    w, info = afm.ic_weights(r["ic"], spec)
    assert same(r["weights"].cpu().numpy(), w.cpu().numpy())
    assert same(r["weights_info"].cpu().numpy(), info.cpu().numpy())
    hw = r["weights"].cpu().numpy()
    assert np.isfinite(hw[20:]).all()
    assert (hw[20:, 3] == (0.0 if method != "equal" else 1 / 6)).all()     # 'd' has no IC
    if method != "maxir":                                   # and the restatement of the weights
        rw, ri = R.ic_weights_ref(r["ic"].cpu().numpy(), spec.q, spec.code, spec.window,
                                  spec.embargo, spec.min_periods)
        assert same(hw, rw) and same(r["weights_info"].cpu().numpy(), ri)
    out, cnt = afm.combine_grid(g["base"], np.arange(g["K"]), r["rows_idx"], r["nrows"],
                                r["dates_idx"], r["weights"], T=g["T"], lda=g["lda"])
    comp = r["composite"].cpu().numpy()
    assert same(comp, out.cpu().numpy()) and same(r["composite_cnt"].cpu().numpy(),
                                                  cnt.cpu().numpy())
    assert np.isfinite(comp).sum() > 1000
    one = afm.screen_grid(r["composite"][None].contiguous(), [0], g["close"], g["price_bits"],
                          g["row_bits"], A=g["A"], dates_idx=r["dates_idx"])
    assert same(r["composite_ic"].cpu().numpy(), one["ic"].cpu().numpy()[:, 0, :])
    assert same(r["composite_stats"].cpu().numpy(), one["stats"].cpu().numpy()[0])
    assert r["composite_ic"].shape == (nd, 3) and r["composite_stats"].shape == (3, 5)
    if method == "icir":                                    # 'a', 'b', 'f' carry the return
        best = np.nanmax(np.abs(r["stats"].cpu().numpy()[:, 0, 1]))
        assert abs(r["composite_stats"].cpu().numpy()[0, 1]) > 0.8 * best


def test_screen_grid_combine_reads_what_the_ic_read(grids):
    import afm
    from afm.xsprep import XsPrep
    g = grids
    spec = spec_of("ic")
    p = XsPrep("mad", neutralize=True)
    r = screen(g, combine=spec, prep=p, groups=g["groups"], ngroups=4)
    out, cnt = afm.combine_grid(r["prep_out"], np.arange(g["K"]), r["rows_idx"], r["nrows"],
                                r["dates_idx"], r["weights"], T=g["T"], lda=g["lda"])
    assert same(r["composite"].cpu().numpy(), out.cpu().numpy())
    plain = screen(g, combine=spec)
    assert not same(r["composite"].cpu().numpy(), plain["composite"].cpu().numpy())
    # the rank ICs feed the weights with corr_method='spearman'
    s = screen(g, combine=spec, corr_method="spearman")
    w, _ = afm.ic_weights(s["ic"], spec)
    assert same(s["weights"].cpu().numpy(), w.cpu().numpy())
    assert not same(s["ic"].cpu().numpy(), plain["ic"].cpu().numpy())
    assert not same(s["weights"].cpu().numpy(), plain["weights"].cpu().numpy())
    one = afm.screen_grid(s["composite"][None].contiguous(), [0], g["close"], g["price_bits"],
                          g["row_bits"], A=g["A"], dates_idx=s["dates_idx"],
                          corr_method="spearman")
    assert same(s["composite_ic"].cpu().numpy(), one["ic"].cpu().numpy()[:, 0, :])


def test_combine_none_changes_nothing(grids):
    g = grids
    bufs = {}
    a = screen(g, bufs=bufs)
    keys = set(bufs)
    b = screen(g)
    assert set(a) == set(b) == {"ic", "stats", "ir_year", "nrows", "rows_idx", "dates_idx", "years",
                                "year0"}
    for k in ("ic", "stats", "ir_year", "nrows"):
        assert same(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    used = np.arange(g["lda"])[None, :] < a["nrows"].cpu().numpy()[:, None]
    assert same(a["rows_idx"].cpu().numpy()[used], b["rows_idx"].cpu().numpy()[used])
    c = screen(g, bufs=bufs, combine=spec_of())
    assert same(c["ic"].cpu().numpy(), b["ic"].cpu().numpy())
    assert set(bufs) - keys == {"weights", "weights_info", "composite", "composite_cnt",
                                "composite_ic", "composite_stats", "composite_scratch"}
    assert not [k for k in keys if "weights" in k or "composite" in k]
    with pytest.raises(ValueError, match="ascending"):
        screen(g, combine=spec_of(), dates_idx=c["dates_idx"][::-1])
    with pytest.raises(TypeError):
        screen(g, combine="icir")


def test_factor_screen_frames_and_combine_factors(ragged, grids):
    import afm
    df, price, g = ragged["df"], ragged["price"], grids
    spec = spec_of("icir", return_type="return_2")
    fs = afm.FactorScreen(df.copy(), price.copy(), combine=spec).run()
    r = fs._res
    ic = r["ic"].cpu().numpy()
    nd, K = ic.shape[0], len(NAMES)
    rw, _ = R.ic_weights_ref(ic, spec.q, spec.code, spec.window, spec.embargo, spec.min_periods)
    have = ~np.isnan(rw).all(axis=1)
    dts = g["dates"][r["dates_idx"]]
    wd = fs.weights_df
    assert list(wd.columns) == ["date", "factor", "weight"] and len(wd) == have.sum() * K
    assert (wd["date"].to_numpy() == np.repeat(dts[have], K)).all()
    assert list(wd["factor"]) == NAMES * int(have.sum())
    assert same(wd["weight"].to_numpy(), rw[have].reshape(-1))
    assert 0 < have.sum() < nd and not have[:spec.embargo + spec.min_periods - 1].any()
    # the composite over the screen's rows
    sent = np.full((g["T"], g["lda"]), np.nan)
    ro, rc = R.combine_ref(g["host_base"], list(range(K)), r["dates_idx"],
                           r["rows_idx"].cpu().numpy(), r["nrows"].cpu().numpy(), rw, sent,
                           np.zeros((g["T"], g["lda"]), dtype=np.int32))
    want = pd.Series(ro[g["st"], g["sa"]], index=df.index, name="composite").dropna()
    assert fs.composite.name == "composite" and fs.composite.index.names == ["date", "id"]
    assert fs.composite.index.equals(want.index) and len(want) > 500
    assert same(fs.composite.to_numpy(), want.to_numpy())
    cs = fs.composite_summary
    assert list(cs.columns) == ["Type", "n", "mean", "std", "IR", "t"]
    assert list(cs["Type"]) == fs.return_type and cs["n"].dtype == np.int64
    assert same(cs[["mean", "std", "IR", "t"]].to_numpy(),
                r["composite_stats"].cpu().numpy()[:, 1:])
    # the frame-level function
    got = afm.combine_factors(df, price, weights=spec)
    assert got.equals(fs.composite)
    sub = afm.combine_factors(df, price, columns=["a", "b", "f"], weights=spec)
    fs3 = afm.FactorScreen(df, price, columns=["a", "b", "f"], combine=spec).run()
    assert sub.equals(fs3.composite) and not sub.equals(got.loc[sub.index])
    with pytest.raises(ValueError, match="price_data"):
        afm.combine_factors(df, weights=spec)


def test_combine_factors_with_static_weights(ragged):
    """A mapping name -> weight: sum w x / sum |w| over the finite cells, as given -- against the
    pandas expression within 4 ulp (the same ascending order of columns; measured on MI355X: 0
    ulp)."""
    import afm
    df = ragged["df"]
    wmap = {"a": 0.5, "b": -0.25, "c": 1.0, "e": 2.0, "f": 0.0}
    got = afm.combine_factors(df, weights=wmap)
    cols = list(wmap)
    x = df[cols].replace([np.inf, -np.inf], np.nan)
    w = pd.Series(wmap)
    live = x.notna() & (w != 0)
    num = (x * w).where(live).sum(axis=1)
    den = (live * w.abs()).sum(axis=1)
    want = (num / den)[live.any(axis=1)].rename("composite")
    assert got.name == "composite" and got.index.equals(want.index)
    ulp = np.abs(got.to_numpy() - want.to_numpy()) / np.spacing(np.abs(want.to_numpy()))
    print(f"combine_factors, static weights: largest distance from pandas {ulp.max():.1f} ulp")
    assert ulp.max() <= 4
    two = afm.combine_factors(df, columns=["a", "c"], weights=wmap)
    x2 = x[["a", "c"]]
    want2 = ((x2 * w[["a", "c"]]).sum(axis=1) / (x2.notna() * w[["a", "c"]].abs()).sum(axis=1))
    assert np.allclose(two.to_numpy(), want2[x2.notna().any(axis=1)].to_numpy(), rtol=1e-15)
    with pytest.raises(ValueError, match="lack a weight"):
        afm.combine_factors(df, columns=["a", "d"], weights=wmap)


# ---- Pipeline.factor_screen --------------------------------------------------------------------
def test_pipeline_factor_screen_with_combine():
    import torch
    import afm
    from afm import _lib
    from afm.factors import COL
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.synthetic import make_panel
    torch.cuda.set_device(0)
    grid = afm.PanelGrid.from_panel(make_panel(300, 700, seed=11, tradable_p=0.9))
    pipe = Pipeline(grid, PipelineConfig(**SPLIT))
    pipe.step()
    torch.cuda.synchronize()
    before = pipe.summary()
    names = [pipe.features[i] for i in (0, 5, 11, 17, 23, pipe.p - 1)]
    spec = afm.ICWeights("maxir", window=40, shrink=0.3)
    plain = pipe.factor_screen("train", columns=names)
    got = pipe.factor_screen("train", columns=names, combine=spec)
    assert set(got) == set(plain) | {"weights", "weights_info", "composite_ic", "composite_stats",
                                     "composite_dev", "composite_t0"}
    for k in set(plain) - {"features"}:
        assert same(np.asarray(plain[k]), np.asarray(got[k])), k
    sp, T, lda, nch = pipe.sp, pipe.T, pipe.lda, pipe.nch
    rb, pb = torch.zeros_like(pipe.zrows), torch.zeros_like(pipe.alldf)
    _lib.run("afm_row_bits", nch, lda, pipe.zrows, None, None, 0, sp.tr1, rb)
    _lib.run("afm_row_bits", nch, lda, pipe.alldf, None, None, 0, sp.tr1, pb)
    cols = np.array([COL[n] for n in names], np.int32)
    zcols = np.array([pipe.features.index(n) for n in names], np.int32)
    w1 = (sp.tr1 + 63) // 64
    years = np.asarray(grid.dates).astype("datetime64[Y]").astype(np.int64) + 1970
    hand = afm.screen_grid(pipe.out[0, :sp.tr1], cols, grid.close[:sp.tr1], pb[:w1], rb[:w1],
                           A=grid.A, zs=pipe.zs, zcols=zcols, col_stride=T * lda,
                           year=years[:sp.tr1], combine=spec)
    for k in ("ic", "weights", "weights_info", "composite_ic", "composite_stats"):
        assert same(got[k], hand[k].cpu().numpy()), k
    assert got["composite_t0"] == 0
    assert same(got["composite_dev"].cpu().numpy(), hand["composite"].cpu().numpy())
    assert np.isfinite(got["weights"][60:]).all() and np.isfinite(got["composite_ic"][60:]).any()
    assert (got["weights_info"][60:, 0] == len(names)).all()
    after = pipe.summary()                                  # the step's results are untouched
    assert before.keys() == after.keys()
    for k in before:
        assert same(np.asarray(before[k]), np.asarray(after[k])), k
    with pytest.raises(ValueError, match="ascending"):
        afm.screen_grid(pipe.out[0, :sp.tr1], cols, grid.close[:sp.tr1], pb[:w1], rb[:w1],
                        A=grid.A, zs=pipe.zs, zcols=zcols, col_stride=T * lda,
                        dates_idx=hand["dates_idx"][[3, 2, 5]], combine=spec)
