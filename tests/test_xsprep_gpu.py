"""The cross-sectional preprocessing end to end on a ragged frame (40 ids x 120 dates x 6 columns
with a group_id): ``preprocess_factors`` and ``prep_info_df`` against the restatements of
tests/xsprep_ref.py (the order statistics and the output of a chain without sums bit for bit, the
rest within max(4 E64, 16 * 2^-53 * max(1, max |ref|)) of the long-double one, per date and
column); ``FactorScreen(df, prices, prep=p, groups=g)`` against the screen of the preprocessed
frame, bit for bit; ``prep=None`` against a second plain run; ``Pipeline.factor_screen(prep=p)``
against ``screen_grid`` called by hand."""
import numpy as np
import pandas as pd
import pytest

import xsprep_ref as X
from helpers import same
from test_sharded import SPLIT

pytestmark = pytest.mark.gpu

NAMES = list("abcdef")


@pytest.fixture(scope="module")
def ragged():
    """120 dates, 40 ids, price rows with p = 0.9, factor rows a subset; 'a' clean, 'b' rounded,
    'c' with NaN and inf cells, 'd' constant, 'e' = 1e6 + noise, 'f' on a 1e-4 scale with
    outliers; group_id: six sectors, one id without a sector (NaN)."""
    rng = np.random.default_rng(23)
    T, A = 120, 40
    dates = np.asarray(np.busday_offset(np.datetime64("2019-03-01"), np.arange(T), roll="forward"),
                       dtype="datetime64[ns]")
    ids = 500 + 7 * np.arange(A)
    present = rng.random((T, A)) < 0.9
    close = 30 * np.exp(np.cumsum(rng.normal(0, 0.02, (T, A)), axis=0))
    inframe = present & (rng.random((T, A)) < 0.85)
    F = rng.normal(size=(6, T, A))
    F[1] = np.round(F[1], 1)
    F[2][rng.random((T, A)) < 0.1] = np.nan
    F[2][rng.random((T, A)) < 0.03] = np.inf
    F[3] = 1.5
    F[4] = 1e6 + F[4]
    F[5] = 1e-4 * F[5] * np.where(rng.random((T, A)) < 0.05, 40.0, 1.0)
    sector = rng.integers(0, 6, size=A).astype(np.float64)
    sector[11] = np.nan
    tt, aa = np.nonzero(inframe)
    idx = pd.MultiIndex.from_arrays([dates[tt], ids[aa]], names=["date", "id"])
    df = pd.DataFrame({c: F[j, tt, aa] for j, c in enumerate(NAMES)}, index=idx)
    pt, pa = np.nonzero(present)
    price = pd.DataFrame({"close_price": close[pt, pa]},
                         index=pd.MultiIndex.from_arrays([dates[pt], ids[pa]]))
    return dict(df=df, price=price, groups=pd.Series(sector[aa], index=idx, name="group_id"))


def codes_of(groups):
    c, u = pd.factorize(groups.to_numpy(), sort=False)
    return c, len(u)


def frame_ref(df, groups, p):
    """The restatement per (date, column) -> out64 / outld frames, info64 / infold / E64 keyed by
    (date, column)."""
    from afm.xsprep import XsPrep
    assert isinstance(p, XsPrep)
    codes, G = codes_of(groups) if p.neutralize else (None, 0)
    p_lo, p_hi = p.params
    o64, old = df.copy(), df.copy()
    info = {}
    pos = pd.Series(np.arange(len(df)), index=df.index)
    for d, rows in pos.groupby(level="date"):
        r = rows.to_numpy()
        for c in df.columns:
            it = X.item(df[c].to_numpy()[r], None if codes is None else codes[r], G, p.mode, p_lo,
                        p_hi, p.flags)
            o64.iloc[r, df.columns.get_loc(c)] = it["out64"]
            old.iloc[r, df.columns.get_loc(c)] = it["outld"]
            info[(d, c)] = it
    return o64, old, info


def preps():
    from afm.xsprep import XsPrep
    return {"default": XsPrep(), "mad": XsPrep("mad", standardize=False),
            "chain": XsPrep("mad", neutralize=True),
            "quantile": XsPrep("quantile", quantiles=(0.05, 0.95), neutralize=True,
                               standardize=False)}


@pytest.mark.parametrize("which", ["default", "mad", "chain", "quantile"])
def test_preprocess_factors_against_the_restatement(ragged, which):
    import afm
    p = preps()[which]
    df, groups = ragged["df"], ragged["groups"]
    got = afm.preprocess_factors(df, groups=groups, prep=p)
    assert got.index.equals(df.index) and list(got.columns) == NAMES
    o64, old, info = frame_ref(df, groups, p)
    assert (got.isna().to_numpy() == old.isna().to_numpy()).all()
    if which == "mad":                                      # order statistics only: bit for bit
        assert same(got.to_numpy(), o64.to_numpy())
    pos = pd.Series(np.arange(len(df)), index=df.index)
    worst = {}
    for d, rows in pos.groupby(level="date"):
        r = rows.to_numpy()
        for c in NAMES:
            ref = old[c].to_numpy()[r]
            if np.isfinite(ref).any():
                err = float(np.nanmax(np.abs(got[c].to_numpy()[r] - ref)))
                e64 = info[(d, c)]["E64"]
                if e64 > 0 and err / e64 > worst.get(c, (0.0,))[0]:
                    worst[c] = (err / e64, err, e64, int(np.isfinite(ref).sum()))
                assert err <= X.tolerance(e64, ref), (which, d, c, err)
    print(f"preprocess_factors {which}: largest |engine - longdouble| / E64 per column (ratio, "
          f"error, E64, rows): {worst}")
    assert got["d"].isna().all() == p.standardize          # the constant column has no z-score
    if p.neutralize:                                        # the id without a sector is missing
        nosec = groups.isna().to_numpy()
        assert nosec.any() and got[nosec].isna().all().all()
        assert not got[~nosec]["a"].isna().any()


def test_preprocess_factors_frame_interface(ragged):
    import afm
    from afm.xsprep import XsPrep
    df, groups = ragged["df"], ragged["groups"]
    p = XsPrep("mad", neutralize=True)
    want = afm.preprocess_factors(df, groups=groups, prep=p)
    named = df.copy()
    named.insert(2, "group_id", groups.map({0.0: "bank", 1.0: "tech", 2.0: "oil", 3.0: "food",
                                            4.0: "auto", 5.0: "air"}))     # labels of any dtype
    got = afm.preprocess_factors(named, groups="group_id", prep=p)
    assert list(got.columns) == list(named.columns) and got["group_id"].equals(named["group_id"])
    assert got[NAMES].equals(want)
    sub = afm.preprocess_factors(named, columns=["f", "a"], groups="group_id", prep=p)
    assert sub[["f", "a"]].equals(want[["f", "a"]]) and sub["b"].equals(named["b"])
    shuffled = groups.sample(frac=1.0, random_state=1)      # a Series is aligned on the index
    assert afm.preprocess_factors(df, groups=shuffled, prep=p).equals(want)
    plain = afm.preprocess_factors(df)                      # XsPrep(): the z-score across the date
    assert plain.equals(afm.preprocess_factors(df, prep=XsPrep()))
    with pytest.raises(ValueError, match="needs groups"):
        afm.preprocess_factors(df, prep=p)
    with pytest.raises(TypeError):
        afm.preprocess_factors(df, prep="mad")


@pytest.mark.parametrize("method", ["pearson", "spearman"])
def test_factor_screen_with_prep_is_the_screen_of_the_preprocessed_frame(ragged, method):
    import afm
    from afm.xsprep import XsPrep
    df, price, groups = ragged["df"], ragged["price"], ragged["groups"]
    p = XsPrep("mad", neutralize=True)
    kw = dict(corr_method=method, layers=True, xcorr=True)
    one = afm.FactorScreen(df.copy(), price.copy(), prep=p, groups=groups, **kw).run()
    two = afm.FactorScreen(afm.preprocess_factors(df, groups=groups, prep=p), price.copy(),
                           **kw).run()
    assert len(one.ic_df) > 1000
    for name in ("ic_df", "ir_df", "summary", "port_ret_df", "layer_summary", "factor_corr",
                 "factor_corr_abs", "factor_corr_n", "redundant_pairs"):
        assert getattr(one, name).equals(getattr(two, name)), name
    for rt in one.return_type:
        assert one.layered_ret_dfs[rt].equals(two.layered_ret_dfs[rt]), rt
        assert one.ls_ret_dfs[rt].equals(two.ls_ret_dfs[rt]), rt
    for k in ("ic", "stats", "ir_year", "layer_mean", "layer_cnt", "port", "xcorr", "xcorr_stats"):
        assert same(one._res[k].cpu().numpy(), two._res[k].cpu().numpy()), k
    assert not hasattr(two, "prep_info_df") and "prep_info" not in two._res
    raw = afm.FactorScreen(df.copy(), price.copy(), **kw).run()
    assert not one.summary.equals(raw.summary)              # the preprocessing matters
    named = df.copy()
    named["group_id"] = groups
    three = afm.FactorScreen(named, price.copy(), prep=p, groups="group_id", **kw).run()
    assert three.columns == NAMES and three.ic_df.equals(one.ic_df)


def test_prep_info_df_against_the_restatement(ragged):
    import afm
    from afm.xsprep import XsPrep
    df, price, groups = ragged["df"], ragged["price"], ragged["groups"]
    p = XsPrep("mad", neutralize=True)
    fs = afm.FactorScreen(df.copy(), price.copy(), prep=p, groups=groups).run()
    pi = fs.prep_info_df
    assert list(pi.columns) == ["date", "factor", "n", "lo", "hi", "n_lo", "n_hi", "mean", "std"]
    dts = pd.DatetimeIndex(fs._res["dates"][fs._res["dates_idx"]])
    assert len(pi) == len(dts) * 6 and len(dts) > 100
    assert list(pi["factor"][:6]) == NAMES and (pi["date"].to_numpy()[::6] == dts.values).all()
    assert pi["n"].dtype == np.int64 and pi["n_lo"].dtype == np.int64
    _, _, info = frame_ref(df, groups, p)
    ref64 = np.array([info[(d, c)]["info64"] for d, c in zip(pi["date"], pi["factor"])])
    refld = np.array([info[(d, c)]["infold"] for d, c in zip(pi["date"], pi["factor"])])
    got = pi[["n", "lo", "hi", "n_lo", "n_hi", "mean", "std"]].to_numpy(np.float64)
    assert same(got[:, :5], ref64[:, :5])
    assert (pi["n_lo"] + pi["n_hi"]).sum() > 0 and pi["n"].max() <= 40
    for j in (5, 6):
        a, b, e = got[:, j], refld[:, j], np.abs(ref64[:, j] - refld[:, j])
        assert (np.isnan(a) == np.isnan(b)).all()
        ok = ~np.isnan(b)
        bound = np.maximum(4 * e[ok], 16 * X.EPS * np.maximum(1.0, np.abs(b[ok])))
        assert (np.abs(a[ok] - b[ok]) <= bound).all(), j


def test_without_prep_nothing_changes(ragged):
    import afm
    df, price = ragged["df"], ragged["price"]
    kw = dict(layers=True, xcorr=True)
    a = afm.FactorScreen(df.copy(), price.copy(), **kw).run()
    b = afm.FactorScreen(df.copy(), price.copy(), prep=None, groups=None, **kw).run()
    for name in ("ic_df", "ir_df", "summary", "port_ret_df", "layer_summary", "factor_corr"):
        assert getattr(a, name).equals(getattr(b, name)), name
    assert set(a._res) == set(b._res) and not {"prep_info", "prep_out"} & set(a._res)
    assert not hasattr(a, "prep_info_df")
    bufs = {}
    from afm.grid import pack_bits
    import torch
    dev = torch.device("cuda", 0)
    T, lda = 8, 64
    close = torch.rand((T, lda), dtype=torch.float64, device=dev) + 1.0
    bits = pack_bits(torch.ones((T, lda), dtype=torch.bool, device=dev))
    base = torch.randn((2, T, lda), dtype=torch.float64, device=dev)
    afm.screen_grid(base, np.arange(2), close, bits, bits, A=lda, bufs=bufs)
    assert not [k for k in bufs if k.startswith("prep")]    # not a buffer


def test_pipeline_factor_screen_with_prep():
    import torch
    import afm
    from afm import _lib
    from afm.factors import COL
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.sharded import EmulatedComm
    from afm.synthetic import make_panel
    from afm.xsprep import XsPrep, factorize_groups
    torch.cuda.set_device(0)
    panel = make_panel(300, 700, seed=11, tradable_p=0.9)
    grid = afm.PanelGrid.from_panel(panel)
    assert same(grid.group, panel.group_id)
    pipe = Pipeline(grid, PipelineConfig(**SPLIT))
    pipe.step()
    torch.cuda.synchronize()
    before = pipe.summary()
    names = [pipe.features[i] for i in (0, 5, 11, 17, 23, pipe.p - 1)]
    p = XsPrep("mad", neutralize=True)
    plain = pipe.factor_screen("train", columns=names)
    got = pipe.factor_screen("train", columns=names, prep=p)
    assert set(got) == set(plain) | {"prep_info"}
    again = pipe.factor_screen("train", columns=names)
    for k in set(plain) - {"features"}:                     # prep=None: what it gave before
        assert same(np.asarray(plain[k]), np.asarray(again[k])), k
    assert not same(got["ic"], plain["ic"]) and same(got["nrows"], plain["nrows"])
    # screen_grid by hand
    sp, T, lda, nch = pipe.sp, pipe.T, pipe.lda, pipe.nch
    rb, pb = torch.zeros_like(pipe.zrows), torch.zeros_like(pipe.alldf)
    _lib.run("afm_row_bits", nch, lda, pipe.zrows, None, None, 0, sp.tr1, rb)
    _lib.run("afm_row_bits", nch, lda, pipe.alldf, None, None, 0, sp.tr1, pb)
    codes, G = factorize_groups(grid.group)
    gdev = torch.full((lda,), -1, dtype=torch.int32, device=pipe.out.device)
    gdev[:grid.A] = torch.from_numpy(codes).to(gdev.device)
    cols = np.array([COL[n] for n in names], np.int32)
    zcols = np.array([pipe.features.index(n) for n in names], np.int32)
    w1 = (sp.tr1 + 63) // 64
    years = np.asarray(grid.dates).astype("datetime64[Y]").astype(np.int64) + 1970
    hand = afm.screen_grid(pipe.out[0, :sp.tr1], cols, grid.close[:sp.tr1], pb[:w1], rb[:w1],
                           A=grid.A, zs=pipe.zs, zcols=zcols, col_stride=T * lda,
                           year=years[:sp.tr1], prep=p, groups=gdev, ngroups=G)
    for k in ("ic", "stats", "ir_year", "prep_info"):
        assert same(got[k], hand[k].cpu().numpy()), k
    assert same(got["dates_idx"], hand["dates_idx"])
    # prep_info against the restatement on a few dates: the z values on the split's z rows
    out, zs = pipe.out.cpu().numpy(), pipe.zs.cpu().numpy()
    rows = afm.unpack_bits(rb, T).cpu().numpy()
    for i in np.linspace(0, len(got["dates_idx"]) - 1, 5).astype(int):
        t = int(got["dates_idx"][i])
        idx = np.flatnonzero(rows[t])
        for k, (c, zc) in enumerate(zip(cols, zcols)):
            with np.errstate(all="ignore"):
                x = (out[c, t, idx] - zs[zc, idx, 0]) * zs[zc, idx, 1]
            it = X.item(x, codes[idx], G, 1, *p.params, p.flags)
            assert same(got["prep_info"][i, k, :5], it["info64"][:5]), (t, names[k])
            for j in (5, 6):
                e = abs(it["info64"][j] - it["infold"][j])
                assert abs(got["prep_info"][i, k, j] - it["infold"][j]) <= \
                    max(4 * e, 16 * X.EPS * max(1.0, abs(it["infold"][j]))), (t, names[k], j)
            o = hand["prep_out"][k, t].cpu().numpy()
            assert (np.isnan(o[idx]) == np.isnan(it["outld"])).all()
            assert np.isnan(np.delete(o, idx)).all()
            ok = ~np.isnan(it["outld"])
            if ok.any():
                assert np.abs(o[idx][ok] - it["outld"][ok]).max() <= \
                    X.tolerance(it["E64"], it["outld"])
    # other labels, given by hand; the default needs the grid's
    lab = np.array(["s%d" % (a % 5) for a in range(grid.A)], dtype=object)
    other = pipe.factor_screen("train", columns=names, prep=p, groups=lab)
    assert not same(other["ic"], got["ic"])
    with pytest.raises(ValueError, match="one label per"):
        pipe.factor_screen("train", columns=names, prep=p, groups=lab[:-1])
    after = pipe.summary()                                  # the step's results are untouched
    for k in before:
        assert same(np.asarray(before[k]), np.asarray(after[k])), k
    two = Pipeline(grid, PipelineConfig(**SPLIT), EmulatedComm(2, 0))
    with pytest.raises(NotImplementedError):
        two.factor_screen(prep=p)


def test_panel_grid_group_from_frame():
    """``PanelGrid.from_frame`` keeps a ``group_id`` column as the grid's ``group`` where every
    security has one label; labels that change over time (or no column) leave it None."""
    import afm
    rng = np.random.default_rng(4)
    dates = pd.bdate_range("2021-01-04", periods=5)
    ids = np.array([30, 10, 20, 40])
    sector = {30: 7, 10: 3, 20: 7, 40: 1}
    rows = [(d, i) for d in dates for i in ids if rng.random() < 0.8]
    df = pd.DataFrame({"data_date": [r[0] for r in rows], "security_id": [r[1] for r in rows]})
    for c in ("close_price", "volume", "ret1d", "excess_ret1d"):
        df[c] = rng.random(len(df)) + 1.0
    assert set(df["security_id"]) == set(ids)
    plain, _, _ = afm.PanelGrid.from_frame(df)
    assert plain.group is None
    df["group_id"] = df["security_id"].map(sector)
    grid, _, _ = afm.PanelGrid.from_frame(df)
    assert list(grid.ids) == [10, 20, 30, 40] and list(grid.group) == [3, 7, 7, 1]
    moved = df.copy()
    mine = moved.index[moved["security_id"] == 10]
    assert len(mine) >= 2
    moved.loc[mine[-1], "group_id"] = 9
    assert afm.PanelGrid.from_frame(moved)[0].group is None
