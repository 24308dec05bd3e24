"""The network ensembles through the public interface: Pipeline.mlp_fit / mlp_predict on the
resident panel of the small synthetic chain of tests/test_gbt_gpu.py, and afm.MLPRegressor on a
frame -- against tests/mlp_ref.py run on the host copy of the same rows (z = (x - mu) * (1/sd)
from the pipeline's own train-window statistics, as the kernels read it), within the trajectory
tolerance measured by the reference on those rows."""
import numpy as np
import pandas as pd
import pytest

import mlp_ref as R

pytestmark = pytest.mark.gpu

GBT = dict(n_rounds=6, max_depth=3, eta=0.2, reg_lambda=1.0, min_child_weight=2.0, max_bin=32)
KW = dict(hidden=(32, 16), epochs=2, lr=1e-3, seeds=(1, 2))


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
        fresh.mlp_fit()
    pipe = Pipeline(grid, cfg)
    pipe.step()
    torch.cuda.synchronize()
    assert pipe.sp.dup and pipe.sp.tr1 == 190 and pipe.sp.v1 == 240
    rows = afm.unpack_bits(pipe.zrows, pipe.T).cpu().numpy()[:, :pipe.lda]
    out = pipe.out.cpu().numpy()
    zs = pipe.zs.cpu().numpy()
    feat = pipe.feat.cpu().numpy()

    def design(t0, t1, idx):
        t, a = np.nonzero(rows[t0:t1])
        t = t + t0
        X = (out[feat[idx]][:, t, a].T - zs[idx][:, a, 0].T) * zs[idx][:, a, 1].T
        return t, a, X, out[afm.factors.TARGET][t, a]
    gbt_model = pipe.gbt_fit(afm.GBTParams(**GBT), rows="train+valid")
    feats = pipe.selected_features(gbt_model)
    model = pipe.mlp_fit(afm.MLPParams(**KW), features=feats)
    torch.cuda.synchronize()
    return panel, grid, pipe, design, gbt_model, feats, model


def reference(pipe, design, feats, model):
    """The host rows of the fit and the reference's fp64 and longdouble fits of every member."""
    from afm.mlp import glorot_init
    sp = pipe.sp
    idx = [pipe.features.index(f) for f in feats]
    tt, ta, Xt, yt = design(0, sp.tr1, idx)
    et, ea, Xe, ye = design(sp.tr1 - 1, sp.v1, idx)
    ok_t, ok_e = np.isfinite(yt), np.isfinite(ye)
    t, a = np.r_[tt[ok_t], et[ok_e]], np.r_[ta[ok_t], ea[ok_e]]
    X, y = np.r_[Xt[ok_t], Xe[ok_e]], np.r_[yt[ok_t], ye[ok_e]]
    n_train, n_eval = int(ok_t.sum()), int(ok_e.sum())
    shape = (len(idx), *model.params.hidden)
    fits = []
    for seed, lr in zip(model.params.seeds, model.params.lrs):
        kw = dict(lr=lr, batch=model.params.batch_size, epochs=model.params.epochs)
        th0 = glorot_init(shape[0], shape[1:], seed)
        fits.append((R.fit(th0, X, y, n_train, n_eval, shape, **kw),
                     R.fit(th0, X, y, n_train, n_eval, shape, dtype=R.LD, **kw)))
    return t, a, X, y, n_train, n_eval, shape, fits


def test_pipeline_fit_against_the_reference(chain):
    panel, grid, pipe, design, gbt_model, feats, model = chain
    sp = pipe.sp
    assert 1 <= len(feats) <= len(pipe.features) and model.features == feats
    t, a, X, y, n_train, n_eval, shape, fits = reference(pipe, design, feats, model)
    assert n_train > 5000 and n_eval > 500
    # the row lists: train = the dates [0, tr1), eval = [tr1 - dup, v1) -- train_end is in both
    assert np.array_equal(pipe.mlp["rows_t"].cpu().numpy(), t)
    assert np.array_equal(pipe.mlp["rows_a"].cpu().numpy(), a)
    assert (pipe.mlp["n_train"], pipe.mlp["n_eval"]) == (n_train, n_eval)
    assert t[:n_train].max() == sp.tr1 - 1 and t[n_train:].min() == sp.tr1 - 1
    assert t[n_train:].max() == sp.v1 - 1
    assert np.array_equal(pipe.mlp["X"][:, :len(y)].cpu().numpy().T, X)
    assert np.array_equal(pipe.mlp["y"][:len(y)].cpu().numpy(), y)
    assert model.theta.shape == (2, R.param_count(*shape)) and model.evals.shape == (2, 2, 2, 6)
    for m, (f64, ld) in enumerate(fits):
        s = float(np.abs(f64["snaps"].astype(R.LD) - ld["snaps"]).max())
        tau = 64 * max(s, R.U * float(np.abs(ld["theta"]).max()))
        err = float(np.abs(model.theta[m].astype(R.LD) - ld["theta"]).max())
        print("member", m, "steps", len(ld["steps"]), "s", s, "tau", tau, "gpu - longdouble", err)
        assert s < 1e-9 and err <= tau
        assert model.snaps[m, -1].tobytes() == model.theta[m].tobytes()
        # evals_frame: the metrics of moments that sit within the image of tau
        fr = model.evals_frame(m)
        from afm.gbt import metrics
        rm, ic = metrics(ld["evals"].astype(np.float64))
        assert fr["n_train"].tolist() == [n_train] * 2 and fr["n_valid"].tolist() == [n_eval] * 2
        assert np.abs(fr["train_rmse"].to_numpy() - rm[:, 0]).max() <= 1e-10
        assert np.abs(fr["valid_rmse"].to_numpy() - rm[:, 1]).max() <= 1e-10
        assert np.abs(fr["valid_ic"].to_numpy() - ic[:, 1]).max() <= 1e-8
        assert model.best_epoch[m] == int(np.argmin(rm[:, 1])) + 1
    assert model.theta[0].tobytes() != model.theta[1].tobytes()


def test_pipeline_predict_plane_frame_and_members(chain):
    import afm
    panel, grid, pipe, design, gbt_model, feats, model = chain
    sp = pipe.sp
    idx = [pipe.features.index(f) for f in feats]
    shape = (len(idx), *model.params.hidden)
    tt, ta, Xt, _ = design(sp.s0, pipe.T, idx)
    planes = [pipe.mlp_predict(model, member=m).cpu().numpy() for m in (0, 1)]
    mean = pipe.mlp_predict(model).cpu().numpy()
    for m, plane in enumerate(planes):
        assert plane.shape == tuple(pipe.pred.shape)
        f, E = R.forward_bound(model.theta[m], Xt, shape)
        assert (np.abs(plane[tt, ta].astype(R.LD) - f) <= E).all()
        rest = np.ones(plane.shape, bool)
        rest[tt, ta] = False
        assert np.isnan(plane[rest]).all() and np.isfinite(plane[tt, ta]).all()
    assert np.array_equal(np.isnan(mean), np.isnan(pipe.pred.cpu().numpy()))
    both = np.stack([planes[0][tt, ta], planes[1][tt, ta]])
    assert np.abs(mean[tt, ta] - both.mean(axis=0)).max() <= 4 * R.U * np.abs(both).max()
    df = pipe.mlp_predict(model, frame=True)
    gdf = pipe.gbt_predict(gbt_model, frame=True)
    assert list(df.columns) == ["pred"] and df.index.names == ["date", "id"]
    assert df.index.equals(gdf.index) and len(df) == len(tt) > 1000
    t, a = np.nonzero(~np.isnan(mean[:, :pipe.A]))
    assert np.array_equal(df["pred"].to_numpy(), mean[t, a])
    v = panel.valid[:, :panel.A]
    pt, pa = np.nonzero(v)
    px = pd.DataFrame({"close_price": panel.close[pt, pa]}, index=pd.MultiIndex.from_arrays(
        [np.asarray(panel.dates)[pt], np.asarray(panel.ids)[pa]]))
    an = afm.AlphaSignalAnalyzer(df, "pred", px)
    an.run()


def test_pipeline_errors(chain):
    import afm
    panel, grid, pipe, design, gbt_model, feats, model = chain
    with pytest.raises(ValueError, match="unknown features"):
        pipe.mlp_fit(afm.MLPParams(**KW), features=feats + ["no_such_column"])
    with pytest.raises(ValueError):
        pipe.mlp_fit(afm.MLPParams(**KW), features=[])
    with pytest.raises(TypeError):
        pipe.mlp_fit({"epochs": 2})
    with pytest.raises(TypeError):
        pipe.mlp_fit(afm.MLPParams(**KW), features="alpha")
    with pytest.raises(TypeError):
        pipe.mlp_predict(gbt_model)
    with pytest.raises(ValueError):
        pipe.mlp_predict(model, member=2)
    with pytest.raises(ValueError):                        # all columns with the widest layers
        pipe.mlp_fit(afm.MLPParams(hidden=(128, 64)))
    from types import SimpleNamespace
    from afm.pipeline import Pipeline
    with pytest.raises(NotImplementedError):
        Pipeline.mlp_fit(SimpleNamespace(W=2))
    with pytest.raises(NotImplementedError):
        Pipeline.mlp_predict(SimpleNamespace(W=2), model)


def test_regressor_on_a_frame_restore_best_and_npz_round_trip(tmp_path):
    import afm
    from afm.mlp import glorot_init, predict_dense
    rng = np.random.default_rng(8)
    n, nv, p = 500, 150, 5
    cols = [f"x{j}" for j in range(p)]
    X = pd.DataFrame(rng.standard_normal((n + nv, p)), columns=cols)
    y = pd.Series(0.3 * X["x1"] * (X["x3"] > 0) + 0.05 * rng.standard_normal(n + nv))
    kw = dict(hidden=(16, 16), epochs=4, lr=(1e-2, 3e-2), batch_size=64, seeds=(3, 4))
    m = afm.MLPRegressor(**kw).fit(X[:n], y[:n], eval_set=[(X[n:], y[n:])])
    shape = (p, 16, 16)
    Xh, yh = X.to_numpy(), y.to_numpy()
    for k, (seed, lr) in enumerate(zip(kw["seeds"], kw["lr"])):
        th0 = glorot_init(p, (16, 16), seed)
        a = R.fit(th0, Xh, yh, n, nv, shape, lr=lr, batch=64, epochs=4)
        b = R.fit(th0, Xh, yh, n, nv, shape, lr=lr, batch=64, epochs=4, dtype=R.LD)
        s = float(np.abs(a["snaps"].astype(R.LD) - b["snaps"]).max())
        tau = 64 * max(s, R.U * float(np.abs(b["theta"]).max()))
        assert s < 1e-9 and np.abs(m.model_.theta[k].astype(R.LD) - b["theta"]).max() <= tau
        f, E = R.forward_bound(m.model_.theta[k], Xh[n:], shape)
        assert (np.abs(m.predict(X[n:], member=k).astype(R.LD) - f) <= E).all()
    ev = m.model_.evals_frame(0)
    assert ev["n_train"].iloc[0] == n and ev["n_valid"].iloc[0] == nv
    assert ev["valid_rmse"].iloc[-1] < ev["valid_rmse"].iloc[0]          # it learns
    assert m.n_features_in_ == p and list(m.feature_names_in_) == cols
    assert m.model_.features == cols and m.best_epoch_.tolist() == m.model_.best_epoch.tolist()
    mean = m.predict(X[n:])
    both = np.stack([m.predict(X[n:].to_numpy(), member=k) for k in (0, 1)])
    assert np.abs(mean - both.mean(axis=0)).max() <= 4 * R.U * np.abs(both).max()
    path = tmp_path / "mlp.npz"
    m.model_.save(path)
    back = afm.MLPModel.load(path)
    assert back.params == m.model_.params and back.features == cols
    assert predict_dense(back, X[n:]).tobytes() == mean.tobytes()
    # restore_best: the same fit, theta = the snapshot of the epoch of lowest validation rmse
    best = afm.MLPRegressor(restore_best=True, **kw).fit(X[:n], y[:n], eval_set=(X[n:], y[n:]))
    assert best.model_.snaps.tobytes() == m.model_.snaps.tobytes()
    for k, e in enumerate(best.best_epoch_):
        assert best.model_.theta[k].tobytes() == m.model_.snaps[k, e - 1].tobytes()
    rm = np.stack([best.model_.evals_frame(k)["valid_rmse"].to_numpy() for k in (0, 1)])
    assert best.best_epoch_.tolist() == (np.argmin(rm, axis=1) + 1).tolist()
    with pytest.raises(ValueError):
        m.predict(X[cols[:3]])
    with pytest.raises(ValueError):
        m.predict(X[:n], member=5)
