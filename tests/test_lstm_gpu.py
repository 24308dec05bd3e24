"""The LSTM ensembles through the public interface: Pipeline.lstm_fit / lstm_predict on the resident
panel of the small synthetic chain of tests/test_mlp_gpu.py -- the reference's layout (every feature
a step) and windows of the last dates of a security -- and afm.LSTMRegressor on arrays."""
import numpy as np
import pandas as pd
import pytest

import lstm_ref as R
from afm.factors import TARGET

pytestmark = pytest.mark.gpu

KW = dict(hidden=(8, 4), epochs=2, lr=1e-3, seeds=(1, 2), batch_size=512)
FEATS = 5          # the first columns of the pipeline's features


@pytest.fixture(scope="module")
def chain():
    import torch
    import afm
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.synthetic import make_panel
    panel = make_panel(100, 300, seed=5, tradable_p=0.9)
    grid = afm.PanelGrid.from_panel(panel)
    d = np.asarray(grid.dates).astype("datetime64[D]")
    cfg = PipelineConfig(train_end=str(d[189]), valid_end=str(d[239]), window=40)
    fresh = Pipeline(grid, cfg)
    with pytest.raises(ValueError, match="step"):
        fresh.lstm_fit()
    pipe = Pipeline(grid, cfg)
    pipe.step()
    torch.cuda.synchronize()
    feats = list(pipe.features[:FEATS])
    flat = pipe.lstm_fit(afm.LSTMParams(**KW), features=feats)
    flat_res = dict(pipe.lstm)
    win = pipe.lstm_fit(afm.LSTMParams(**KW), features=feats, lookback=3)
    win_res = dict(pipe.lstm)
    torch.cuda.synchronize()
    rows = afm.unpack_bits(pipe.zrows, pipe.T).cpu().numpy()[:, :pipe.lda].astype(bool)
    return panel, pipe, feats, flat, flat_res, win, win_res, rows


def host_z(pipe, idx):
    """z [len(idx)][T][lda] on the host, as the kernels read it: (x - mu) * (1 / sd)."""
    out, zs, feat = pipe.out.cpu().numpy(), pipe.zs.cpu().numpy(), pipe.feat.cpu().numpy()
    return (out[feat[idx]] - zs[idx][:, None, :, 0]) * zs[idx][:, None, :, 1]


def test_reference_layout_planes_are_the_mlp_planes(chain):
    import torch
    panel, pipe, feats, flat, res, win, win_res, rows = chain
    idx = [pipe.features.index(f) for f in feats]
    n, n_pad = int(res["rows_t"].numel()), int(res["X"].shape[2])
    assert tuple(res["X"].shape) == (FEATS, 1, n_pad) and flat.lookback is None
    assert (flat.T, flat.d) == (FEATS, 1) and flat.features == feats
    want = pipe._mlp_planes(idx, res["rows_t"], res["rows_a"], n_pad)
    assert torch.equal(res["X"].view(FEATS, n_pad), want)
    # the rows are mlp_fit's: every z-score row of the dates [0, tr1), then [tr1 - dup, v1)
    sp = pipe.sp
    t, a = np.nonzero(rows[:sp.v1])
    y = pipe.out.cpu().numpy()[TARGET]
    tr, ev = t < sp.tr1, t >= sp.tr1 - 1
    tt, aa = np.r_[t[tr], t[ev]], np.r_[a[tr], a[ev]]
    ok = np.isfinite(y[tt, aa])
    assert np.array_equal(res["rows_t"].cpu().numpy(), tt[ok])
    assert np.array_equal(res["rows_a"].cpu().numpy(), aa[ok])
    assert res["n_train"] == int(ok[:tr.sum()].sum()) and res["n_train"] + res["n_eval"] == n
    assert flat.theta.shape == (2, R.param_count(1, 8, 4)) and flat.evals.shape == (2, 2, 2, 6)
    assert (flat.evals[:, :, 0, 0] == res["n_train"]).all()
    assert (flat.evals[:, :, 1, 0] == res["n_eval"]).all()
    assert flat.theta[0].tobytes() != flat.theta[1].tobytes() and np.isfinite(flat.theta).all()


def test_lookback_windows_against_a_host_gather(chain):
    panel, pipe, feats, flat, flat_res, win, res, rows = chain
    L, sp = 3, pipe.sp
    idx = [pipe.features.index(f) for f in feats]
    assert win.lookback == L and (win.T, win.d) == (L, FEATS)
    full = rows.copy()
    full[1:] &= rows[:-1]
    full[2:] &= rows[:-2]
    full[:L - 1] = False
    t, a = np.nonzero(full[:sp.v1])
    y = pipe.out.cpu().numpy()[TARGET]
    tr, ev = t < sp.tr1, t >= sp.tr1 - 1
    tt, aa = np.r_[t[tr], t[ev]], np.r_[a[tr], a[ev]]
    ok = np.isfinite(y[tt, aa])
    tt, aa = tt[ok], aa[ok]
    assert 0 < len(tt) < int(flat_res["rows_t"].numel())           # some rows have no full window
    assert np.array_equal(res["rows_t"].cpu().numpy(), tt)
    assert np.array_equal(res["rows_a"].cpu().numpy(), aa)
    z = host_z(pipe, idx)
    X = res["X"].cpu().numpy()
    assert X.shape[:2] == (L, FEATS)
    for s in range(L):
        want = z[:, tt - (L - 1 - s), aa]                           # [FEATS][n]
        assert np.array_equal(X[s][:, :len(tt)], want), s
    assert not X[:, :, len(tt):].any()
    # the fit against the restatement on those rows
    n_train, n_eval = res["n_train"], res["n_eval"]
    from afm.lstm import lstm_init
    Xh = np.ascontiguousarray(X[:, :, :len(tt)].transpose(2, 0, 1))
    yh = res["y"].cpu().numpy()[:len(tt)]
    shape = (L, FEATS, 8, 4)
    kw = dict(lr=1e-3, batch=512, epochs=2)
    th0 = lstm_init(FEATS, (8, 4), 1)
    b = R.fit(th0, Xh, yh, n_train, n_eval, shape, dtype=R.LD, **kw)
    s = max(float(np.abs(R.fit(th0, Xh, yh, n_train, n_eval, shape, **kw, **v)["theta"].astype(R.LD)
                         - b["theta"]).max()) for v in R.variants())
    tau = 64 * max(s, R.U * float(np.abs(b["theta"]).max()))
    err = float(np.abs(win.theta[0].astype(R.LD) - b["theta"]).max())
    print("steps", len(b["steps"]), "s", s, "tau", tau, "gpu - longdouble", err)
    assert s < 1e-9 and err <= tau


def test_predict_plane_frame_and_members(chain):
    import afm
    panel, pipe, feats, flat, flat_res, win, win_res, rows = chain
    sp = pipe.sp
    full = rows.copy()
    full[1:] &= rows[:-1]
    full[2:] &= rows[:-2]
    for model, mask in ((flat, rows), (win, full)):
        tt, ta = np.nonzero(mask[sp.s0:])
        tt = tt + sp.s0
        planes = [pipe.lstm_predict(model, member=m).cpu().numpy() for m in (0, 1)]
        mean = pipe.lstm_predict(model).cpu().numpy()
        for plane in planes:
            assert plane.shape == tuple(pipe.pred.shape)
            rest = np.ones(plane.shape, bool)
            rest[tt, ta] = False
            assert np.isnan(plane[rest]).all() and np.isfinite(plane[tt, ta]).all()
        both = np.stack([planes[0][tt, ta], planes[1][tt, ta]])
        assert np.abs(mean[tt, ta] - both.mean(axis=0)).max() <= 4 * R.U * np.abs(both).max()
        assert np.array_equal(np.isnan(mean), np.isnan(planes[0]))
        assert planes[0][tt, ta].tobytes() != planes[1][tt, ta].tobytes()
    # the windowed prediction against the restatement on a host gather
    idx = [pipe.features.index(f) for f in feats]
    z = host_z(pipe, idx)
    Xh = np.stack([z[:, tt - (2 - s), ta].T for s in range(3)], axis=1)       # [n][3][FEATS]
    f = R.forward(win.theta[0], Xh, (3, FEATS, 8, 4), dtype=R.LD)
    sF = max(float(np.abs(R.forward(win.theta[0], Xh, (3, FEATS, 8, 4), **v).astype(R.LD) - f).max())
             for v in R.variants())
    assert np.abs(planes[0][tt, ta].astype(R.LD) - f).max() <= 64 * max(sF, R.U * float(np.abs(f).max()))
    df = pipe.lstm_predict(flat, frame=True)
    assert list(df.columns) == ["pred"] and df.index.names == ["date", "id"]
    mean = pipe.lstm_predict(flat).cpu().numpy()
    t, a = np.nonzero(~np.isnan(mean[:, :pipe.A]))
    assert len(df) == len(t) > 1000 and np.array_equal(df["pred"].to_numpy(), mean[t, a])
    v = panel.valid[:, :panel.A]
    pt, pa = np.nonzero(v)
    px = pd.DataFrame({"close_price": panel.close[pt, pa]}, index=pd.MultiIndex.from_arrays(
        [np.asarray(panel.dates)[pt], np.asarray(panel.ids)[pa]]))
    an = afm.AlphaSignalAnalyzer(df, "pred", px)
    an.run()
    out = pipe.out.cpu().numpy()
    idx = pd.MultiIndex.from_arrays([np.asarray(panel.dates)[pt], np.asarray(panel.ids)[pa]])
    hist = pd.DataFrame({"target": out[afm.factors.TARGET][pt, pa]}, index=idx).dropna()
    all_df = pd.DataFrame({"in_trading_universe": np.where(panel.tradable[pt, pa], "Y", "N"),
                           "close_price": panel.close[pt, pa],
                           "tmr_ret1d": out[afm.factors.TMR][pt, pa]},
                          index=idx.set_names(["data_date", "security_id"]))
    pm = afm.PortfolioManager(df, hist, all_df, top_n=5, window=60)
    pm.calculate_portfolio()
    assert len(pm.portfolio_value["Portfolio"]) > 1
    assert np.isfinite(np.asarray(pm.portfolio_value["Portfolio"], dtype=np.float64)).all()


def test_pipeline_errors(chain):
    import afm
    panel, pipe, feats, flat, flat_res, win, win_res, rows = chain
    with pytest.raises(ValueError, match="unknown features"):
        pipe.lstm_fit(afm.LSTMParams(**KW), features=feats + ["no_such_column"])
    with pytest.raises(TypeError):
        pipe.lstm_fit({"epochs": 2})
    for lb in (0, 257, 2.5):
        with pytest.raises(ValueError, match="lookback"):
            pipe.lstm_fit(afm.LSTMParams(**KW), features=feats, lookback=lb)
    with pytest.raises(ValueError):                        # 97 columns as inputs of a step
        pipe.lstm_fit(afm.LSTMParams(**KW), lookback=2)
    with pytest.raises(TypeError):
        pipe.lstm_predict(None)
    with pytest.raises(ValueError):
        pipe.lstm_predict(flat, member=2)


def test_regressor_2d_3d_restore_best_and_npz_round_trip(tmp_path):
    import afm
    from afm.lstm import predict_sequences
    rng = np.random.default_rng(8)
    n, nv, p = 300, 100, 6
    X = rng.standard_normal((n + nv, p))
    y = 0.3 * X[:, 1] * (X[:, 3] > 0) + 0.05 * rng.standard_normal(n + nv)
    kw = dict(hidden=(8, 8), epochs=3, lr=(1e-2, 3e-2), batch_size=64, seeds=(3, 4))
    m2 = afm.LSTMRegressor(**kw).fit(X[:n], y[:n], eval_set=[(X[n:], y[n:])])
    m3 = afm.LSTMRegressor(**kw).fit(X[:n, :, None], y[:n], eval_set=(X[n:, :, None], y[n:]))
    assert m2.model_.theta.tobytes() == m3.model_.theta.tobytes()
    assert m2.model_.evals.tobytes() == m3.model_.evals.tobytes()
    assert m2.predict(X[n:]).tobytes() == m3.predict(X[n:, :, None]).tobytes()
    assert m2.model_.lookback is None and m3.model_.lookback == p and m2.n_features_in_ == p
    ev = m2.model_.evals_frame(0)
    assert ev["n_train"].iloc[0] == n and ev["n_valid"].iloc[0] == nv
    frame = afm.LSTMRegressor(**kw).fit(pd.DataFrame(X[:n], columns=list("abcdef")), pd.Series(y[:n]))
    assert list(frame.feature_names_in_) == list("abcdef")
    assert frame.model_.features == list("abcdef") and frame.model_.lookback is None
    mean = m2.predict(X[n:])
    both = np.stack([m2.predict(X[n:], member=k) for k in (0, 1)])
    assert np.abs(mean - both.mean(axis=0)).max() <= 4 * R.U * np.abs(both).max()
    path = tmp_path / "lstm.npz"
    m2.model_.save(path)
    back = afm.LSTMModel.load(path)
    assert back.params == m2.model_.params and back.lookback is None
    assert predict_sequences(back, X[n:]).tobytes() == mean.tobytes()
    best = afm.LSTMRegressor(restore_best=True, **kw).fit(X[:n], y[:n], eval_set=(X[n:], y[n:]))
    assert best.model_.snaps.tobytes() == m2.model_.snaps.tobytes()
    for k, e in enumerate(best.best_epoch_):
        assert best.model_.theta[k].tobytes() == m2.model_.snaps[k, e - 1].tobytes()
    rm = np.stack([best.model_.evals_frame(k)["valid_rmse"].to_numpy() for k in (0, 1)])
    assert best.best_epoch_.tolist() == (np.argmin(rm, axis=1) + 1).tolist()
    with pytest.raises(ValueError):
        m2.predict(X[:, :3])
    with pytest.raises(ValueError):
        m2.predict(X[:n], member=5)
