"""Boosted trees through the public interface: Pipeline.gbt_fit / gbt_predict / selected_features
on the resident panel of a small synthetic chain, and afm.GBTRegressor on a frame -- trees, fit
values and predictions bit for bit against tests/gbt_ref.py run on the host copy of the same rows
(z = (x - mu) * (1/sd) from the pipeline's own train-window statistics, as the kernels read it)."""
import numpy as np
import pandas as pd
import pytest

import gbt_ref as R

pytestmark = pytest.mark.gpu

KW = dict(n_rounds=6, max_depth=3, eta=0.2, reg_lambda=1.0, min_child_weight=2.0, max_bin=32)


@pytest.fixture(scope="module")
def chain():
    import torch
    import afm
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.synthetic import make_panel
    panel = make_panel(100, 300, seed=5, tradable_p=0.9)
    grid = afm.PanelGrid.from_panel(panel)
    d = np.asarray(grid.dates).astype("datetime64[D]")
    pipe = Pipeline(grid, PipelineConfig(train_end=str(d[189]), valid_end=str(d[239]), window=40))
    pipe.step()
    torch.cuda.synchronize()
    assert pipe.sp.dup and pipe.sp.tr1 == 190 and pipe.sp.v1 == 240
    # the host copy of the design: z of every feature on the z-score rows, the raw target
    rows = afm.unpack_bits(pipe.zrows, pipe.T).cpu().numpy()[:, :pipe.lda]
    out = pipe.out.cpu().numpy()
    zs = pipe.zs.cpu().numpy()
    feat = pipe.feat.cpu().numpy()

    def design(t0, t1):
        t, a = np.nonzero(rows[t0:t1])
        t = t + t0
        X = (out[feat][:, t, a].T - zs[:pipe.p, a, 0].T) * zs[:pipe.p, a, 1].T
        return t, a, X, out[afm.factors.TARGET][t, a]
    return panel, grid, pipe, design


@pytest.mark.parametrize("mode", ["train", "train+valid"])
def test_pipeline_fit_and_predict_against_the_reference(chain, mode):
    import torch
    import afm
    panel, grid, pipe, design = chain
    sp = pipe.sp
    prm = afm.GBTParams(**KW)
    model = pipe.gbt_fit(prm, rows=mode)
    torch.cuda.synchronize()
    t, a, X, y = design(0, sp.v1)
    assert np.isfinite(X).all() and np.isfinite(y).all() and len(y) > 5000
    if mode == "train":
        w = (t < sp.tr1).astype(np.int32)
        assert (w == 0).sum() > 500
    else:
        w = 1 + (t == sp.tr1 - 1).astype(np.int32)
        assert (w == 2).sum() > 50
    want = R.fit(X, y, w, **KW)
    assert np.array_equal(pipe.gbt["rows_t"].cpu().numpy(), t)
    assert np.array_equal(pipe.gbt["rows_a"].cpu().numpy(), a)
    assert np.array_equal(pipe.gbt["w"].cpu().numpy(), w)
    for k in ("cuts", "ncuts", "feat", "bin", "thr", "val"):
        assert getattr(model, k).tobytes() == want[k].tobytes(), k
    assert pipe.gbt["F"].cpu().numpy().tobytes() == want["F"].tobytes()
    assert np.array_equal(pipe.gbt["bins"].cpu().numpy(), want["bins"])
    assert (model.feat >= 0).sum() > 20 and model.features == list(pipe.features)
    # the per-round frame: rmse and IC of the training rows and of the rows only evaluated
    ev = model.evals
    rm, ic = R.metrics(R.moments(want["F"], y, w)[0])
    assert abs(ev["train_rmse"].iloc[-1] - rm) <= 1e-12 and abs(ev["train_ic"].iloc[-1] - ic) <= 1e-9
    assert ev["n_train"].iloc[0] == (w > 0).sum() and ev["n_valid"].iloc[0] == (w == 0).sum()
    if mode == "train":
        rm, ic = R.metrics(R.moments(want["F"], y, w)[1])
        assert abs(ev["valid_ic"].iloc[-1] - ic) <= 1e-9
        assert model.best_round == int(np.nanargmax(ev["valid_ic"].to_numpy())) + 1
    else:
        assert ev["valid_ic"].isna().all() and model.best_round == KW["n_rounds"]
    # the test dates: the tree walk over the panel, NaN off the rows, like pipe.pred
    tt, ta, Xt, _ = design(sp.s0, pipe.T)
    for nt in (None, 2, 0):
        plane = pipe.gbt_predict(model, n_trees=nt).cpu().numpy()
        assert plane.shape == tuple(pipe.pred.shape)
        ref = np.full(plane.shape, np.nan)
        ref[tt, ta] = R.predict(Xt, want["feat"], want["thr"], want["val"], 0.0, n_trees=nt)
        assert plane.tobytes() == ref.tobytes()
    assert np.array_equal(np.isnan(plane), np.isnan(pipe.pred.cpu().numpy()))


def test_frame_feeds_the_analyzer_and_selected_features(chain):
    import afm
    panel, grid, pipe, design = chain
    model = pipe.gbt_fit(afm.GBTParams(**KW), rows="train+valid")
    plane = pipe.gbt_predict(model).cpu().numpy()
    df = pipe.gbt_predict(model, frame=True)
    assert list(df.columns) == ["pred"] and df.index.names == ["date", "id"]
    t, a = np.nonzero(~np.isnan(plane))
    assert len(df) == len(t) > 1000
    assert np.array_equal(df["pred"].to_numpy(), plane[t, a])
    assert np.array_equal(df.index.get_level_values("id").to_numpy(), np.asarray(grid.ids)[a])
    v = panel.valid[:, :panel.A]
    pt, pa = np.nonzero(v)
    px = pd.DataFrame({"close_price": panel.close[pt, pa]}, index=pd.MultiIndex.from_arrays(
        [np.asarray(panel.dates)[pt], np.asarray(panel.ids)[pa]]))
    an = afm.AlphaSignalAnalyzer(df, "pred", px)
    an.run()
    # selected_features: the most-split columns united with the Lasso's, in FEATURES order
    beta = pipe.lasso_beta.cpu().numpy()
    lasso = {f for f, b in zip(pipe.features, beta[1:]) if b != 0}
    for k in (10, 1):
        sel = pipe.selected_features(model, k=k)
        assert set(sel) == set(model.top_features(k)) | lasso
        assert sel == [f for f in pipe.features if f in set(sel)]
    cnt = model.importance("weight")
    top = model.top_features(10)
    assert len(top) == min(10, int((cnt > 0).sum())) >= 1   # the synthetic target has one strong twin
    assert [cnt[pipe.features.index(f)] for f in top] == sorted(cnt, reverse=True)[:len(top)]
    with pytest.raises(ValueError):
        pipe.gbt_fit(rows="valid")
    with pytest.raises(TypeError):
        pipe.gbt_predict(object())


def test_regressor_on_a_frame_and_npz_round_trip(tmp_path):
    import afm
    rng = np.random.default_rng(8)
    n, nv, p = 700, 200, 5
    cols = [f"x{j}" for j in range(p)]
    X = pd.DataFrame(rng.standard_normal((n + nv, p)), columns=cols)
    y = pd.Series(0.04 * np.sign(X["x1"]) * (X["x3"] > 0) + 0.01 * rng.standard_normal(n + nv))
    sw = rng.choice([1, 1, 2], size=n)
    kw = dict(n_rounds=8, max_depth=2, eta=0.3, max_bin=64, base_score=0.002)
    m = afm.GBTRegressor(**kw).fit(X[:n], y[:n], eval_set=[(X[n:], y[n:])], sample_weight=sw)
    w = np.r_[sw, np.zeros(nv)].astype(np.int32)
    want = R.fit(X.to_numpy(), y.to_numpy(), w, **kw)
    for k in ("cuts", "ncuts", "feat", "bin", "thr", "val"):
        assert getattr(m.model_, k).tobytes() == want[k].tobytes(), k
    assert m.train_prediction_.tobytes() == want["F"][:n].tobytes()
    assert m.predict(X[:n]).tobytes() == want["F"][:n].tobytes()
    assert m.predict(X[n:]).tobytes() == want["F"][n:].tobytes()
    assert m.predict(X[n:].to_numpy(), n_trees=3).tobytes() == \
        R.predict(X[n:].to_numpy(), want["feat"], want["thr"], want["val"], 0.002, 3).tobytes()
    assert m.n_features_in_ == p and list(m.feature_names_in_) == cols
    assert m.model_.features == cols and m.best_round_ == m.model_.best_round
    imp = m.feature_importances_
    assert abs(imp.sum() - 1) < 1e-12 and set(np.argsort(-imp)[:2]) == {1, 3}
    assert m.model_.evals["n_valid"].iloc[0] == nv and m.model_.evals["valid_ic"].iloc[-1] > 0.5
    path = tmp_path / "gbt.npz"
    m.model_.save(path)
    back = afm.GBTModel.load(path)
    assert back.params == m.model_.params and back.features == cols
    from afm.gbt import predict_dense
    assert predict_dense(back, X[n:]).tobytes() == want["F"][n:].tobytes()
    with pytest.raises(ValueError):
        m.predict(X[cols[:3]])
    with pytest.raises(ValueError):
        m.predict(X[:n], n_trees=9)
