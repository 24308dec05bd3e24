"""The risk model through the public interface: Pipeline.risk_fit / book_risk / risk_rebalance on the
resident panel of a small synthetic chain (80 securities x 300 days) against tests/risk_ref.py run on
the downloaded planes, the sums the book rows must satisfy, and the constraints and optimality of
the weights solved from the model's covariance."""
import numpy as np
import pytest

import mv_ref
import risk_ref as R
from helpers import same

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FEATS = ["sd_15", "MOM_38", "corr_15", "RSI_8", "volsd_15"]
TOP_N, HI = 12, 0.2


@pytest.fixture(scope="module")
def chain():
    import torch
    import afm
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.synthetic import make_panel
    grid = afm.PanelGrid.from_panel(make_panel(80, 300, seed=5, tradable_p=0.9))
    d = np.asarray(grid.dates).astype("datetime64[D]")
    cfg = PipelineConfig(train_end=str(d[189]), valid_end=str(d[239]), window=40, top_n=TOP_N,
                         hi=HI)
    fresh = Pipeline(grid, cfg)
    with pytest.raises(ValueError, match="step"):
        fresh.risk_fit()
    pipe = Pipeline(grid, cfg)
    pipe.step()
    torch.cuda.synchronize()
    prm = afm.RiskParams(half_life=30.0, spec_half_life=20.0, min_obs=10, lag=1)
    model = pipe.risk_fit(prm, features=FEATS)
    torch.cuda.synchronize()
    return grid, pipe, prm, model


def host_design(pipe, names, bits):
    import afm
    from afm.factors import COL, TARGET
    out = pipe.out.cpu().numpy()
    mask = afm.unpack_bits(bits, pipe.T).cpu().numpy()[:, :pipe.A].astype(bool)
    X = np.stack([out[COL[f]][:, :pipe.A] for f in names])
    return X, out[TARGET][:, :pipe.A], mask


def check_fit(pipe, model, prm, names, bits):
    X, y, mask = host_design(pipe, names, bits)
    beta, rank = model["beta"].cpu().numpy(), model["rank"].cpu().numpy()
    A = pipe.A
    u = R.residuals(X, y, mask, beta, rank)
    resid = pipe.risk["resid"].cpu().numpy()
    assert same(resid[:, :A], u) and np.isnan(resid[:, A:]).all()
    f, n = R.factor_cov(beta, rank, prm.half_life, prm.min_obs, prm.lag)
    assert same(model["fcov"].cpu().numpy(), f) and same(model["nused"].cpu().numpy(), n)
    s, fl = R.specific(u, prm.spec_hl, prm.min_obs, prm.lag)
    assert same(model["spec"].cpu().numpy()[:, :A], s) and same(model["fill"].cpu().numpy(), fl)
    return X, u, f, s, fl


def test_risk_fit_equals_the_statement(chain):
    import afm
    grid, pipe, prm, model = chain
    assert model.features == FEATS and model.factors == ["intercept"] + FEATS
    assert model.params == prm and len(model.dates) == pipe.T
    X, u, f, s, fl = check_fit(pipe, model, prm, FEATS, pipe.zrows)
    used = model.used
    assert used.sum() > 150 and not used.all()        # the factors' warm-up dates have no rows
    assert np.isfinite(f[-1]).all() and np.isfinite(s[-1]).sum() > 40
    fr, vol = model.factor_returns, model.factor_vol
    assert fr.shape == vol.shape == (pipe.T, 6) and fr[used].notna().all().all()
    assert same(vol.to_numpy(), np.sqrt(np.diagonal(f, axis1=1, axis2=2)))
    c = model.factor_corr(pipe.T - 1).to_numpy()
    assert same(c, c.T) and np.abs(np.diag(c) - 1).max() < 1e-14 and np.abs(c).max() <= 1 + 1e-12
    # the default design (the Fama-MacBeth columns) over the all_df rows
    prm2 = afm.RiskParams(half_life=60.0, min_obs=5, lag=0)
    m2 = pipe.risk_fit(prm2, rows="alldf")
    assert m2.features == list(pipe.cfg.fm_features) and m2["fcov"].shape[1] == 31
    check_fit(pipe, m2, prm2, m2.features, pipe.alldf)
    for bad in (dict(rows="train"), dict(features=["nope"]), dict(features=["sd_15", "sd_15"]),
                dict(features=list(afm.FACTOR_NAMES[:32]))):
        with pytest.raises(ValueError):
            pipe.risk_fit(prm, **bad)
    with pytest.raises(TypeError):
        pipe.risk_fit({"half_life": 3})


def reference_books(pipe, model, reb, names):
    X, _, _ = host_design(pipe, names, pipe.zrows)
    k, ids, w = (reb[key].cpu().numpy() for key in ("k", "books", "weights"))
    rd = pipe.rdates.cpu().numpy()
    fcov, spec, fill = (model[key].cpu().numpy() for key in ("fcov", "spec", "fill"))
    return R.books(X, rd, k, ids, w, fcov, spec[:, :pipe.A], fill, TOP_N)


def test_book_risk_rows(chain, tmp_path):
    import afm
    grid, pipe, prm, model = chain
    frame = pipe.book_risk(model)
    rd = pipe.rdates.cpu().numpy()
    assert len(frame) == pipe.nd == len(rd) and (frame["status"] == 0).all()
    cov, risk, contrib, status = reference_books(pipe, model, pipe.reb, FEATS)
    got = pipe.risk_books
    assert same(got["cov"].cpu().numpy(), cov) and same(got["risk"].cpu().numpy(), risk)
    assert same(got["contrib"].cpu().numpy(), contrib)
    K1 = 6
    for s, book in enumerate(("long", "short", "net")):
        tot, fv, sv = risk[:, s, 0], risk[:, s, 1], risk[:, s, 2]
        assert same(frame[f"{book}_vol"].to_numpy(), np.sqrt(tot))
        assert same(frame[f"{book}_factor_vol"].to_numpy(), np.sqrt(fv))
        assert same(frame[f"{book}_specific_vol"].to_numpy(), np.sqrt(sv))
        assert (tot == fv + sv).all() and (tot > 0).all()
        terms = np.abs(contrib[:, s]).sum(axis=1)
        assert (np.abs(contrib[:, s].sum(axis=1) - fv) <= K1 * U * terms).all()
    # half the difference of two books: ((sigma_L + sigma_S) / 2)^2 bounds the net factor variance
    assert (risk[:, 2, 1] <= np.maximum(risk[:, 0, 1], risk[:, 1, 1]) * (1 + 1e-12)).all()
    con = frame.attrs["contrib"]
    assert con.shape == (pipe.nd, 18) and con.columns[0] == ("long", "intercept")
    assert same(con.to_numpy(), contrib.reshape(pipe.nd, -1))
    # a saved and reloaded model prices the books alike
    path = tmp_path / "risk.npz"
    model.save(path)
    back = afm.RiskModel.load(path, device=pipe.out.device)
    assert back.params == prm and back.features == FEATS
    assert pipe.book_risk(back).equals(frame)
    with pytest.raises(TypeError):
        pipe.book_risk(model.planes)


def test_dates_without_a_forecast_are_flagged_and_keep_their_weights(chain):
    import afm
    grid, pipe, prm, model = chain
    rd = pipe.rdates.cpu().numpy()
    fcov = model["fcov"].clone()
    fcov[rd[: len(rd) // 2].tolist()] = float("nan")  # as before min_obs used dates
    m = afm.RiskModel(prm, FEATS, model.dates, model.ids, dict(model.planes, fcov=fcov))
    frame = pipe.book_risk(m)
    st = frame["status"].to_numpy()
    assert (st[: len(rd) // 2] == 4).all() and st[len(rd) // 2] == 0 and (st[len(rd) // 2:] == 0).all()
    assert frame[st == 4].drop(columns="status").isna().all().all()
    assert frame[st == 0].notna().all().all()
    res = pipe.risk_rebalance(m)
    w, base = res["weights"].cpu().numpy(), pipe.reb["weights"].cpu().numpy()
    rs = res["status"].cpu().numpy()
    assert same(w[st == 4], base[st == 4]) and (rs[st == 4] == 4).all() and not rs[st == 0].any()
    assert same(res["sums"].cpu().numpy()[st == 4], pipe.reb["sums"].cpu().numpy()[st == 4])
    assert not same(w[st == 0], base[st == 0])


@pytest.mark.parametrize("gamma", [0.0, 0.05])
def test_risk_rebalance_weights(chain, gamma):
    from afm.portfolio import pnl_scan
    grid, pipe, prm, model = chain
    res = pipe.risk_rebalance(model, risk_tolerance=gamma)
    k, books, w = (res[key].cpu().numpy() for key in ("k", "books", "weights"))
    assert (k == TOP_N).all() and not res["status"].any() and not res["cov_status"].any()
    for key in ("k", "books", "upos", "usize"):       # the selection is the step's (upos: the
        x, y = res[key].cpu().numpy(), pipe.reb[key].cpu().numpy()       # members' slots)
        assert same(x[..., :TOP_N], y[..., :TOP_N]) if key == "upos" else same(x, y), key
    assert not same(w, pipe.reb["weights"].cpu().numpy())
    ww = w[:, :, :TOP_N]
    assert np.abs(ww.sum(axis=2) - 1).max() < 1e-12 and ww.min() >= 0.0 and ww.max() <= HI
    # the covariance is the statement's on the step's books (the selection is the same)
    cov = reference_books(pipe, model, pipe.reb, FEATS)[0]
    assert same(res["cov"].cpu().numpy(), cov)
    pred = pipe.pred.cpu().numpy()
    rd = pipe.rdates.cpu().numpy()
    worst = 0.0
    for i in range(0, len(rd), 7):
        for s in range(2):
            mu = np.nan_to_num(pred[rd[i], books[i, s, :TOP_N]]) * (1 if s == 0 else -1)
            wo, _ = mv_ref.box_qp_mv(cov[i, s], mu, gamma, 0.0, HI)
            worst = max(worst, np.abs(ww[i, s] - wo).max())
            assert mv_ref.kkt_residual(cov[i, s], mu, gamma, ww[i, s], 0.0, HI) < 1e-9
    print(f"gamma={gamma}: worst |w - ref| {worst:.2e}")
    assert worst < 1e-9
    # sums and the scan follow the new weights
    tmr, close = pipe.tmr.cpu().numpy(), pipe.full.close.cpu().numpy()
    sums = res["sums"].cpu().numpy()
    for i in (0, len(rd) - 1):
        for s in range(2):
            mem = books[i, s, :TOP_N]
            assert np.isclose(sums[i, s], np.nansum(tmr[rd[i], mem] * ww[i, s]), rtol=1e-12,
                              atol=1e-18)
            assert np.isclose(sums[i, 2 + s], (ww[i, s] * close[rd[i], mem]).sum(), rtol=1e-12)
    again = pnl_scan({key: res[key] for key in ("k", "books", "sums", "upos", "usize")},
                     pipe.cfg.v0, pipe.cfg.rate)
    v = res["value"].cpu().numpy()
    assert same(v, again["value"].cpu().numpy()) and v[0] == pipe.cfg.v0 and np.isfinite(v).all()
    assert len(v) == pipe.nd + 1
    if gamma:
        plain = pipe.risk_rebalance(model)
        assert not same(plain["weights"].cpu().numpy(), w)
    with pytest.raises(ValueError):
        pipe.risk_rebalance(model, risk_tolerance=-1.0)
    with pytest.raises(TypeError):
        pipe.risk_rebalance(None)
