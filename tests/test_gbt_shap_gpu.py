"""Attribution through the public interface: afm.GBTRegressor.predict(pred_contribs=True) and
Pipeline.gbt_contribs / selected_features(by="shap") on the small synthetic chain of
tests/test_gbt_gpu.py -- the contributions bit for bit against tests/gbt_shap_ref.py on the host
copy of the same rows, within the derived bound (gbt_shap_ref's docstring) of the Shapley values
by definition, and summing to the predictions."""
import numpy as np
import pandas as pd
import pytest

import gbt_ref as R
import gbt_shap_ref as S
from test_gbt_gpu import KW, chain  # noqa: F401  (the module-scoped pipeline fixture)

pytestmark = pytest.mark.gpu


def test_regressor_pred_contribs_against_the_reference(tmp_path):
    import afm
    from afm.gbt import contribs_dense
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
    cov = S.cover(want["bins"], w, want["feat"], want["bin"])
    model = m.model_
    assert model.cover.dtype == np.int64 and np.array_equal(model.cover, cov)
    assert (cov[:, 0] == w.sum()).all()
    assert model.importance("total_cover")[1] > 0 and model.importance("cover")[1] >= 1
    Xv = X[n:].to_numpy()
    E = S.bound(want["feat"], want["val"], 0.002)
    for nt in (None, 3, 0):
        got = m.predict(X[n:], n_trees=nt, pred_contribs=True)
        assert got.shape == (nv, p + 1) and got.dtype == np.float64
        ref = S.contribs_pinned(Xv, want["feat"], want["thr"], want["val"], cov, 0.002, nt)
        assert got.tobytes() == ref.tobytes()
        exact = S.contribs_by_definition(Xv, want["feat"], want["thr"], want["val"], cov, 0.002, nt)
        assert np.abs(got.astype(np.longdouble) - exact).max() <= 2 * E
        pred = m.predict(X[n:], n_trees=nt)
        assert np.abs(got.astype(np.longdouble).sum(axis=1) - pred).max() <= (p + 1) * 2 * E + E
    assert (got[:, :p] == 0).all() and (got[:, p] == 0.002).all()          # no tree
    # the npz carries the cover; a file written without it loads, and then raises
    path = tmp_path / "gbt.npz"
    model.save(path)
    back = afm.GBTModel.load(path)
    assert np.array_equal(back.cover, cov)
    assert contribs_dense(back, Xv).tobytes() == m.predict(Xv, pred_contribs=True).tobytes()
    back.cover = None
    back.save(path)
    bare = afm.GBTModel.load(path)
    assert bare.cover is None
    with pytest.raises(ValueError, match="cover"):
        contribs_dense(bare, Xv)
    with pytest.raises(ValueError):
        m.predict(X[cols[:3]], pred_contribs=True)
    with pytest.raises(ValueError):
        m.predict(X[:n], n_trees=9, pred_contribs=True)


@pytest.fixture(scope="module")
def fitted(chain):  # noqa: F811
    import torch
    import afm
    panel, grid, pipe, design = chain
    model = pipe.gbt_fit(afm.GBTParams(**KW), rows="train")
    torch.cuda.synchronize()
    return pipe, design, model


def test_pipeline_fit_carries_the_cover(fitted):
    pipe, design, model = fitted
    g = pipe.gbt
    w = g["w"].cpu().numpy()
    cov = S.cover(g["bins"].cpu().numpy(), w, model.feat, model.bin)
    assert np.array_equal(g["cover"].cpu().numpy(), cov) and np.array_equal(model.cover, cov)
    assert (cov[:, 0] == w.sum()).all() and (cov[model.feat != S.ABSENT] >= 2).all()


@pytest.mark.parametrize("split", ["train", "valid", "test"])
def test_gbt_contribs_frames_and_planes(fitted, split):
    pipe, design, model = fitted
    sp, p = pipe.sp, pipe.p
    t0, t1 = {"train": (0, sp.tr1), "valid": (sp.tr1, sp.v1), "test": (sp.s0, pipe.T)}[split]
    res = pipe.gbt_contribs(model, split=split, rows=True)
    assert set(res) == {"by_date", "mean_by_date", "importance", "n", "contrib"}
    names = list(pipe.features) + ["bias"]
    nt = t1 - t0
    for k in ("by_date", "mean_by_date"):
        assert res[k].shape == (nt, p + 1) and list(res[k].columns) == names
        assert list(res[k].index) == list(np.asarray(pipe.full.dates)[t0:t1])
    plane = res["contrib"].cpu().numpy()
    assert plane.shape == (nt, p + 1, pipe.lda)
    # the rows of the split on the host, as the kernels read them
    t, a, X, _ = design(t0, t1)
    assert len(t) > 500
    use = np.zeros((nt, pipe.lda), dtype=bool)
    use[t - t0, a] = True
    assert np.array_equal(~np.isnan(plane[:, 0, :]), use)
    assert np.array_equal(res["n"].to_numpy(), use.sum(axis=1))
    ref = S.contribs_pinned(X, model.feat, model.thr, model.val, model.cover, 0.0)
    got = plane[t - t0, :, a]
    assert got.tobytes() == ref.tobytes()
    E = S.bound(model.feat, model.val, 0.0)
    sub = np.arange(0, len(t), 7)                              # the enumeration on every 7th row
    exact = S.contribs_by_definition(X[sub], model.feat, model.thr, model.val, model.cover, 0.0)
    assert np.abs(got[sub].astype(np.longdouble) - exact).max() <= 2 * E
    pred = R.predict(X, model.feat, model.thr, model.val, 0.0)
    assert np.abs(got.astype(np.longdouble).sum(axis=1) - pred).max() <= (p + 1) * 2 * E + E
    if split == "test":                                        # ... and to gbt_predict's plane
        dev = pipe.gbt_predict(model).cpu().numpy()
        assert np.array_equal(dev[t, a], pred)
    # the frames are the pinned aggregates over the rows; importance their row-weighted mean
    agg, cnt = S.agg_pinned(plane, use)
    with np.errstate(all="ignore"):
        per = agg / cnt[:, None, None].astype(np.float64)
    assert res["by_date"].to_numpy().tobytes() == per[:, :, 1].tobytes()
    assert res["mean_by_date"].to_numpy().tobytes() == per[:, :, 0].tobytes()
    imp = res["importance"]
    assert list(imp.index) != list(pipe.features) and sorted(imp.index) == sorted(pipe.features)
    assert (np.diff(imp.to_numpy()) <= 0).all() and imp.iloc[0] > 0
    by = res["by_date"][list(pipe.features)].to_numpy()
    live = cnt > 0
    wmean = (by[live] * cnt[live, None]).sum(axis=0) / cnt.sum()
    assert np.allclose(imp[list(pipe.features)].to_numpy(), wmean, rtol=1e-12, atol=0)
    # without rows: the same frames, no planes; a prefix of the trees
    lean = pipe.gbt_contribs(model, split=split)
    assert "contrib" not in lean
    assert lean["by_date"].to_numpy().tobytes() == res["by_date"].to_numpy().tobytes()
    two = pipe.gbt_contribs(model, n_trees=2, split=split)
    assert (two["by_date"].to_numpy()[live] != per[live][:, :, 1]).any()


def test_selected_features_by_shap_and_guards(fitted):
    from types import SimpleNamespace
    import afm
    from afm.pipeline import Pipeline
    pipe, design, model = fitted
    beta = pipe.lasso_beta.cpu().numpy()
    lasso = {f for f, b in zip(pipe.features, beta[1:]) if b != 0}
    for split in ("valid", "test"):
        imp = pipe.gbt_contribs(model, split=split)["importance"]
        for k in (10, 1):
            top = [f for f in imp.index[:k] if imp[f] > 0]
            sel = pipe.selected_features(model, k=k, by="shap", split=split)
            assert set(sel) == set(top) | lasso and len(top) >= 1
            assert sel == [f for f in pipe.features if f in set(sel)]
    # a column the trees never split on has no contribution and is never selected by shap
    never = [f for f, c in zip(pipe.features, model.importance("weight")) if c == 0]
    assert never and (imp[never] == 0).all()
    assert pipe.selected_features(model, k=10) == pipe.selected_features(model, k=10, by="weight")
    with pytest.raises(ValueError):
        pipe.selected_features(model, by="gain")
    with pytest.raises(ValueError):
        pipe.gbt_contribs(model, split="all")
    with pytest.raises(TypeError):
        pipe.gbt_contribs(object())
    bare = afm.GBTModel(model.params, model.features, model.feat, model.bin, model.thr, model.val,
                        model.cuts, model.ncuts, model.evals_raw)
    with pytest.raises(ValueError, match="cover"):
        pipe.gbt_contribs(bare)
    other = afm.GBTModel(model.params, model.features[::-1], model.feat, model.bin, model.thr,
                         model.val, model.cuts, model.ncuts, model.evals_raw, cover=model.cover)
    with pytest.raises(ValueError, match="features"):
        pipe.gbt_contribs(other)
    with pytest.raises(NotImplementedError):
        Pipeline.gbt_contribs(SimpleNamespace(W=2), model)
