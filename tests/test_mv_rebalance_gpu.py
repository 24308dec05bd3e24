"""GPU parity of the mean-variance rebalance (afm_rebalance_mv_f64) against tests/mv_ref.py on a
small synthetic panel: rebalance_kernel<32> (top_n = 12) and the 128-name kernel with the
member-major history (top_n = 40), both sources of mu, a moderate and a dominating risk
tolerance; then the same call through PortfolioManager and one Pipeline step."""
import numpy as np
import pandas as pd
import pytest

import mv_ref
from helpers import same

pytestmark = pytest.mark.gpu

T, A, NREB, WINDOW = 120, 96, 20, 60


@pytest.fixture(scope="module")
def panel():
    """96 assets x 120 dates with holes (2 % of the asset-days absent; 0.4 % of the history
    returns, so that the pairwise covariance of 40 names over 60 dates stays positive definite --
    the reference's Cholesky raises otherwise); predictions on the last 20 dates, history on every
    date (each window of 60 dates is full), two common factors in the returns."""
    rng = np.random.default_rng(96)
    dates = np.asarray(np.busday_offset(np.datetime64("2016-01-04"), np.arange(T), roll="forward"),
                       dtype="datetime64[ns]")
    ids = 1000 + 7 * np.arange(A)
    present = rng.random((T, A)) < 0.98
    tt, aa = np.nonzero(present)
    d, i = dates[tt], ids[aa]
    f = rng.normal(0, 0.01, (T, 2))
    full = f @ rng.normal(0, 1, (2, A)) + rng.normal(0, 0.02, (T, A)) * rng.uniform(0.5, 2, A)
    ret = full[tt, aa]
    ht, ha = np.nonzero(present | (rng.random((T, A)) < 0.8))
    close = 50 * np.exp(rng.normal(0, 0.1, len(tt)))
    trad = rng.random(len(tt)) < 0.95
    test_m = tt >= T - NREB
    pred_v = rng.normal(0, 2e-3, test_m.sum())
    pred = pd.DataFrame({"p": pred_v}, index=pd.MultiIndex.from_arrays([d[test_m], i[test_m]]))
    hist = pd.DataFrame({"target": full[ht, ha]},
                        index=pd.MultiIndex.from_arrays([dates[ht], ids[ha]]))
    all_df = pd.DataFrame({"in_trading_universe": np.where(trad, "Y", "N"), "close_price": close,
                           "tmr_ret1d": ret}, index=pd.MultiIndex.from_arrays([d, i]))
    long_args = (d[test_m].astype(np.int64), i[test_m], pred_v, dates[ht].astype(np.int64),
                 ids[ha], full[ht, ha], d.astype(np.int64), i, trad, close, ret)
    return pred, hist, all_df, long_args


@pytest.fixture(scope="module")
def planes(panel):
    from afm.portfolio import PortfolioManager
    pred, hist, all_df, _ = panel
    return PortfolioManager(pred, hist, all_df)._grid()


def run(g, top_n, **kw):
    from afm.portfolio import rebalance
    return rebalance(g["pred"], g["tbits"], g["hist"], g["hbits"], g["close"], g["tmr"],
                     g["rdates"], A=g["A"], top_n=top_n, window=WINDOW, **kw)


def same_outputs(a, b, keys=None):
    """The rebalance outputs of two calls, bit for bit (upos: the members' slots -- the rest of a
    book's row is never written)."""
    k = int(a["k"].max())
    for key in keys or a:
        x, y = a[key].cpu().numpy(), b[key].cpu().numpy()
        if key == "upos":
            x, y = x[..., :k], y[..., :k]
        assert same(x, y), key


def check_against(o, reb, res, ids, top_n):
    k = reb["k"].cpu().numpy()
    books, w = reb["books"].cpu().numpy(), reb["weights"].cpu().numpy()
    assert (reb["status"].cpu().numpy() == 0).all()
    worst = 0.0
    for j in range(len(k)):
        for s in range(2):
            assert ids[books[j, s, :k[j]]].tolist() == o["books"][2 * j + s].tolist(), (j, s)
            worst = max(worst, np.abs(w[j, s, :k[j]] - o["weights"][2 * j + s]).max())
    print(f"top_n={top_n}: worst |w - ref| {worst:.2e}")
    assert worst < 1e-9
    v = res["value"].cpu().numpy()
    assert np.abs(v - o["value"]).max() / o["value"].max() < 1e-12
    to = res["turnover"].cpu().numpy().copy()
    to[0] = 0.0                                            # no positions before the first date
    assert np.abs(to - o["turnover"]).max() <= 1e-9 * max(1.0, o["turnover"].max())


@pytest.mark.parametrize("top_n", [12, 40])
@pytest.mark.parametrize("expected", ["prediction", "history"])
@pytest.mark.parametrize("gamma", [0.05, 5.0])
def test_rebalance_vs_reference(panel, planes, top_n, expected, gamma):
    from afm.portfolio import pnl_scan
    g = planes
    base = run(g, top_n)
    reb = run(g, top_n, risk_tolerance=gamma,
              mu=g["pred"] if expected == "prediction" else "history")
    # selection is untouched
    assert (reb["k"].cpu().numpy() == top_n).all()
    same_outputs(reb, base, ("k", "books", "upos", "usize"))
    o = mv_ref.run_portfolio_mv(*panel[3], top_n=top_n, window=WINDOW, gamma=gamma,
                                expected=expected)
    check_against(o, reb, pnl_scan(reb, rate=1e-4), g["ids"], top_n)
    # the term changes the weights (the test would pass on a solve that ignored it otherwise)
    assert np.abs(reb["weights"].cpu().numpy() - base["weights"].cpu().numpy()).max() > 1e-3


@pytest.mark.parametrize("top_n", [12, 40])
def test_zero_tolerance_is_the_min_variance_rebalance(planes, top_n):
    g = planes
    base = run(g, top_n)
    for mu in (None, g["pred"], "history"):
        reb = run(g, top_n, risk_tolerance=0.0, mu=mu)
        same_outputs(reb, base)
    # and through the new entry point itself
    import torch
    from afm import _lib
    from afm.portfolio import MAX_BOOK
    T_, lda = g["pred"].shape
    nd = int(g["rdates"].numel())
    out = {key: torch.zeros_like(v) for key, v in base.items()}
    out["books"].fill_(-1)
    _lib.run("afm_rebalance_mv_f64", T_, g["A"], lda, g["rdates"], nd, g["pred"], g["tbits"],
             g["hist"], g["hbits"], 0, T_, WINDOW, g["close"], g["tmr"], top_n, 0.0, 0.1,
             g["pred"], 0.0, out["k"], out["books"], out["weights"], out["sums"], out["upos"],
             out["usize"], out["status"])
    assert out["books"].shape[-1] == MAX_BOOK
    same_outputs(out, base)


@pytest.mark.parametrize("gamma", [-1.0, float("nan")])
def test_bad_gamma_is_rejected(planes, gamma):
    from afm._lib import AfmError
    with pytest.raises(AfmError, match="gamma"):
        run(planes, 12, risk_tolerance=gamma, mu="history")


def test_portfolio_manager_follows_the_setting(panel, planes):
    from afm.portfolio import PortfolioManager, pnl_scan
    pred, hist, all_df, long_args = panel
    pm = PortfolioManager(pred, hist, all_df, top_n=12, window=WINDOW, risk_tolerance=0.05,
                          expected="prediction")
    pm.calculate_portfolio()
    reb = run(planes, 12, risk_tolerance=0.05, mu=planes["pred"])
    res = pnl_scan(reb, rate=pm.trading_cost_rate)
    assert same(pm.weights, reb["weights"].cpu().numpy())
    assert same(np.asarray(pm.portfolio_value["Portfolio"], dtype=np.float64),
                res["value"].cpu().numpy())
    o = mv_ref.run_portfolio_mv(*long_args, top_n=12, window=WINDOW, gamma=0.05)
    v = np.asarray(pm.portfolio_value["Portfolio"], dtype=np.float64)
    assert np.abs(v - o["value"]).max() / o["value"].max() < 1e-12
    assert np.abs(np.asarray(pm.turnovers, dtype=np.float64) - o["turnover"]).max() <= \
        1e-9 * max(1.0, o["turnover"].max())
    # the bootstrap follows the same setting: its identity path is calculate_portfolio
    _, got = pm.bootstrap(paths=np.arange(NREB, dtype=np.int32)[None, :])
    assert same(got["value"][0], v)
    # determine_weights: the history mean, the reference's own mean_returns
    from oracle import portfolio as P
    R = mv_ref.make_book(np.random.default_rng(2), 12, 40, True)
    pm2 = PortfolioManager(pred, hist, all_df, hi=0.2, risk_tolerance=0.05)
    wo, _ = mv_ref.box_qp_mv(P.pairwise_cov(R), mv_ref.history_mean(R), 0.05, 0.0, 0.2)
    assert np.abs(pm2.determine_weights(pd.DataFrame(R)) - wo).max() < 1e-9


def test_pipeline_step_uses_the_predictions():
    """One step at world size 1 with the return term: the weights equal, bit for bit, a
    stand-alone rebalance on the pipeline's own planes with mu = the prediction plane."""
    import torch
    import afm
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.portfolio import rebalance
    from afm.synthetic import make_panel
    from test_sharded import SPLIT
    torch.cuda.set_device(0)
    grid = afm.PanelGrid.from_panel(make_panel(300, 700, seed=11, tradable_p=0.9))
    pipe = Pipeline(grid, PipelineConfig(**SPLIT, top_n=20, risk_tolerance=0.05))
    pipe.step()
    torch.cuda.synchronize()
    c, full = pipe.cfg, pipe.full
    kw = dict(A=full.A, top_n=20, window=c.window, h_range=(0, pipe.sp.tr1), lo=c.lo, hi=c.hi)
    alone = rebalance(pipe.pred, full.tbits, pipe.target, pipe.zrows_full, full.close, pipe.tmr,
                      pipe.rdates, risk_tolerance=0.05, mu=pipe.pred, **kw)
    plain = rebalance(pipe.pred, full.tbits, pipe.target, pipe.zrows_full, full.close, pipe.tmr,
                      pipe.rdates, **kw)
    torch.cuda.synchronize()
    assert (pipe.reb["status"].cpu().numpy() == 0).all()
    for key in ("k", "books", "weights", "sums"):
        assert same(pipe.reb[key].cpu().numpy(), alone[key].cpu().numpy()), key
    assert same(pipe.reb["books"].cpu().numpy(), plain["books"].cpu().numpy())
    assert not same(pipe.reb["weights"].cpu().numpy(), plain["weights"].cpu().numpy())
