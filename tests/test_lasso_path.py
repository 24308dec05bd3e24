"""Batched Lasso paths and validation-scored alpha selection: afm_lasso_batch_f64,
afm_gram_score_f64, afm.lasso_path, afm.LassoCV and Pipeline.lasso_cv().

CPU: the restatement the GPU tests lean on (tests/lasso_path_ref.py: the oracle's Gram descent
chained with ``w`` carried; LassoCV rebuilt from per-fold moments) against scikit-learn 1.7.2.
GPU: the kernels against that restatement bit for bit, and the drop-ins against scikit-learn.

Tolerances.  The oracle chain and ``sklearn.lasso_path(precompute=Q, Xy=q)`` run the same Gram
coordinate descent, BLAS reductions against sequential ones: coefficients agree to 1e-9 of
max|coef| at tol 1e-12 (measured 1e-12), and at tol 1e-4 every solve stops on the same sweep.
Fold MSEs are smooth in the coefficients: rel 1e-10 against sklearn for the CPU restatement
(measured 7.6e-14), rel 1e-9 for the GPU drop-in (its moments come from the shifted segment
Grams, not from centered rows).  The refit of ``sklearn.LassoCV`` is the residual-form descent,
so ``coef_`` / ``intercept_`` carry the bars of tests/test_lasso.py: 1e-6 of max|coef| at tol 1e-4,
1e-9 at tol <= 1e-10.  Moment-form scores against row-form numpy: rel 1e-10 for the MSE, abs
1e-10 for R^2 and the IC (both O(1); measured 5e-16).

``alpha_`` "equal": the GPU grid agrees with scikit-learn's to rel 1e-12 (alpha_max comes from
pooled moments), so equality is asserted on the grid position and the value at that bar."""
import functools
import warnings

import numpy as np
import pytest

from lasso_path_ref import (centered, dense_design, geom_alphas, kfold, lasso_cv_ref,
                            oracle_chain, raw_gram)

CV_CASES = [(2000, 20, 4), (1003, 70, 5), (700, 110, 3)]
N_ALPHAS = 12
MAX_ITER = 10000


@functools.lru_cache(maxsize=None)
def _cv_data(n, p):
    return dense_design(n, p, seed=1000 + p)


@functools.lru_cache(maxsize=None)
def _sk_cv(n, p, K, tol, single_split=False):
    from sklearn.linear_model import LassoCV
    X, y = _cv_data(n, p)
    cv = [_time_split(n)] if single_split else K
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LassoCV(alphas=N_ALPHAS, eps=1e-3, cv=cv, tol=tol, max_iter=MAX_ITER).fit(X, y)


def _time_split(n):
    k = (2 * n) // 3
    return np.arange(k), np.arange(k, n)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


# ---- CPU: the restatement against scikit-learn --------------------------------------------------
def test_oracle_chain_matches_sklearn_lasso_path():
    from sklearn.linear_model import lasso_path
    X, y = dense_design(3000, 30, seed=30)
    n, Q, q, yy, xm, ym = centered(X, y)
    Xc, yc = X - xm, y - ym
    alphas = geom_alphas(np.abs(q).max() / n, N_ALPHAS)
    for tol in (1e-12, 1e-4):
        W, info = oracle_chain(Q, q, yy, alphas * n, max_iter=MAX_ITER, tol=tol)
        a, coefs, gaps, iters = lasso_path(Xc, yc, alphas=alphas, precompute=Q, Xy=q, tol=tol,
                                           max_iter=MAX_ITER, return_n_iter=True)
        assert np.array_equal(a, alphas)
        print(f"tol {tol:g}: coef rel {_rel(W.T, coefs):.3g}, n_iter {info[:, 2].astype(int)}")
        if tol == 1e-12:
            assert np.abs(W.T - coefs).max() <= 1e-9 * np.abs(coefs).max()
        else:
            assert info[:, 2].astype(int).tolist() == list(iters)
        assert (W[-1] != 0).sum() >= 5


@pytest.mark.parametrize("n,p,K", CV_CASES)
@pytest.mark.parametrize("tol", [1e-4, 1e-10])
def test_moment_lassocv_matches_sklearn(n, p, K, tol):
    X, y = _cv_data(n, p)
    sk = _sk_cv(n, p, K, tol)
    r = lasso_cv_ref(X, y, N_ALPHAS, kfold(n, K), tol=tol, max_iter=MAX_ITER)
    scale = max(np.abs(sk.coef_).max(), 1e-300)
    print(f"mse rel {_rel(r['mse_path'], sk.mse_path_):.3g}, coef rel "
          f"{np.abs(r['coef'] - sk.coef_).max() / scale:.3g}")
    best = int(np.flatnonzero(sk.alphas_ == sk.alpha_)[0])       # (grids agree to rounding)
    assert r["best"] == best and abs(r["alpha"] / sk.alpha_ - 1) <= 1e-12
    assert r["mse_path"].shape == sk.mse_path_.shape
    assert np.abs(r["mse_path"] / sk.mse_path_ - 1).max() <= 1e-10
    bar = 1e-9 if tol == 1e-10 else 1e-6
    assert np.abs(r["coef"] - sk.coef_).max() <= bar * scale
    assert abs(r["intercept"] - sk.intercept_) <= bar * scale


# ---- GPU: the kernels ---------------------------------------------------------------------------
KERNEL_CASES = [(1, 0), (63, 0), (65, 0), (110, 0), (70, 1)]
N_FIT, N_HELD = 1500, 700
SUBSETS = [slice(0, 1000), slice(250, 1250), slice(500, 1500)]


@functools.lru_cache(maxsize=None)
def _kernel_case(p):
    """Three Grams (row subsets of 1500 generator rows), their centered moments, a 9-alpha grid
    from the largest alpha_max (an all-zero solution included), and the held-out rows."""
    X, y = dense_design(N_FIT + N_HELD, p, seed=p)
    G = np.stack([raw_gram(X[s], y[s]) for s in SUBSETS])
    import oracle
    cm = [oracle.centered_moments(g) for g in G]
    alphas = geom_alphas(max(np.abs(q).max() / n for n, _, q, _ in cm), 9)
    return X, y, G, cm, alphas


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(G, alphas, p, *, nprob, warm, tol, pos, shared=False):
    from afm.regression import lasso_batch
    import torch
    shift = torch.zeros((G.shape[0], p + 2), dtype=torch.float64, device="cuda")
    beta, info = lasso_batch(_dev(G), shift, p, _dev(alphas), nprob=nprob, warm=warm,
                             max_iter=MAX_ITER, tol=tol, positive=bool(pos), shared=shared)
    return beta.cpu().numpy(), info.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("p,pos", KERNEL_CASES)
def test_batch_cold_equals_single_fits(p, pos):
    import torch
    from afm import _lib
    _, _, G, _, alphas = _kernel_case(p)
    beta, info = _batch(G, alphas, p, nprob=3, warm=False, tol=1e-4, pos=pos)
    Gd = _dev(G)
    shift = torch.zeros(p + 2, dtype=torch.float64, device="cuda")
    b1 = torch.empty((3, len(alphas), p + 1), dtype=torch.float64, device="cuda")
    i1 = torch.empty((3, len(alphas), 3), dtype=torch.float64, device="cuda")
    h = _lib.Context.get(0).bind_stream()
    for b in range(3):
        for i, a in enumerate(alphas):
            _lib.check(_lib.lib().afm_lasso_fit_f64(h, _lib.ptr(Gd[b]), _lib.ptr(shift), p,
                                                    float(a), MAX_ITER, 1e-4, pos,
                                                    _lib.ptr(b1[b, i]), _lib.ptr(i1[b, i])))
    assert beta.tobytes() == b1.cpu().numpy().tobytes()
    assert info.tobytes() == i1.cpu().numpy().tobytes()
    assert (beta[:, 0, 1:] == 0).all(axis=1).any()               # an all-zero solution
    assert (beta[:, -1, 1:] != 0).any()
    # one Gram shared by three problems: three identical blocks
    bs, is_ = _batch(G[:1], alphas, p, nprob=3, warm=False, tol=1e-4, pos=pos, shared=True)
    for b in range(3):
        assert bs[b].tobytes() == beta[0].tobytes() and is_[b].tobytes() == info[0].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("p,pos", KERNEL_CASES)
@pytest.mark.parametrize("tol", [1e-4, 1e-10])
def test_batch_warm_equals_oracle_chain(p, pos, tol):
    _, _, G, cm, alphas = _kernel_case(p)
    beta, info = _batch(G, alphas, p, nprob=3, warm=True, tol=tol, pos=pos)
    for b, (n, Q, q, yy) in enumerate(cm):
        W, inf = oracle_chain(Q, q, yy, alphas * n, max_iter=MAX_ITER, tol=tol, positive=pos)
        assert beta[b, :, 1:].tobytes() == W.tobytes()           # signed zeros included
        assert info[b].tolist() == inf.tolist()
        mean = 0.0 + G[b][0] / n                                 # shift + G[0] / n, zero shift
        for i in range(len(alphas)):
            xw = 0.0
            for j in range(p):
                xw = xw + mean[1 + j] * W[i, j]
            assert beta[b, i, 0] == mean[1 + p] - xw


@pytest.mark.gpu
def test_warm_chain_takes_fewer_sweeps_than_cold():
    """A kernel that ignored ``warm`` would pass the comparison above only if it were the oracle
    chain; this pins the point of the chain as well: fewer sweeps in total than cold solves."""
    fewer = []
    for p, pos in KERNEL_CASES:
        _, _, G, _, alphas = _kernel_case(p)
        _, iw = _batch(G, alphas, p, nprob=3, warm=True, tol=1e-4, pos=pos)
        _, ic = _batch(G, alphas, p, nprob=3, warm=False, tol=1e-4, pos=pos)
        print(p, pos, "warm sweeps", iw[:, :, 2].sum(), "cold sweeps", ic[:, :, 2].sum())
        fewer.append(iw[:, :, 2].sum() < ic[:, :, 2].sum())
    assert any(fewer)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [65, 110])
def test_gram_score_matches_rows(p):
    import torch
    from afm.regression import gram_score
    X, y, G, cm, alphas = _kernel_case(p)
    Xtr, ytr = X[:N_FIT], y[:N_FIT]
    Gtr = raw_gram(Xtr, ytr)[None]
    beta, _ = _batch(Gtr, alphas, p, nprob=1, warm=True, tol=1e-4, pos=0)
    zero = np.zeros((1, 1, p + 1))
    zero[0, 0, 0] = ytr.mean()
    models = np.concatenate([zero, beta], axis=1)                # the all-zero model first
    Xh, yh = X[N_FIT:], y[N_FIT:]
    shift = torch.zeros((1, p + 2), dtype=torch.float64, device="cuda")
    out = gram_score(_dev(raw_gram(Xh, yh)[None]), shift, p, _dev(models)).cpu().numpy()[0]
    sst = ((yh - yh.mean()) ** 2).sum()
    for i, m in enumerate(models[0]):
        pred = Xh @ m[1:] + m[0]
        sse = ((yh - pred) ** 2).sum()
        n_, mse, r2, ic = out[i]
        assert n_ == N_HELD
        print(i, mse / (sse / N_HELD) - 1, r2 - (1 - sse / sst))
        assert abs(mse - sse / N_HELD) <= 1e-10 * (sse / N_HELD)
        assert abs(r2 - (1 - sse / sst)) <= 1e-10
        if m[1:].any():
            assert abs(ic - np.corrcoef(pred, yh)[0, 1]) <= 1e-10
        else:
            assert np.isnan(ic)
    assert abs(out[0, 1] - ((yh - ytr.mean()) ** 2).mean()) <= 1e-10 * out[0, 1]
    assert (models[0, -1, 1:] != 0).sum() >= 5


@pytest.mark.gpu
def test_batch_argument_errors():
    import torch
    from afm import _lib
    L = _lib.lib()
    h = _lib.Context.get(0).bind_stream()
    t = torch.zeros(112 * 112, dtype=torch.float64, device="cuda")
    P = _lib.ptr(t)
    for p, nalpha, alphas in ((0, 1, P), (111, 1, P), (3, 0, P), (3, 1, None)):
        rc = L.afm_lasso_batch_f64(h, P, 0, P, 0, p, alphas, nalpha, 1, 1, 10, 1e-4, 0, P, P)
        assert rc == -1 and b"afm_lasso_batch_f64" in L.afm_last_error()     # AFM_E_ARG
    for p, nmodel in ((0, 1), (111, 1), (3, 0)):
        rc = L.afm_gram_score_f64(h, P, 0, P, 0, p, P, nmodel, 1, P)
        assert rc == -1 and b"afm_gram_score_f64" in L.afm_last_error()


# ---- GPU: the drop-ins against scikit-learn -----------------------------------------------------
def _check_cv(m, sk, X, tol):
    scale = max(np.abs(sk.coef_).max(), 1e-300)
    bar = 1e-9 if tol <= 1e-10 else 1e-6
    assert m.alphas_.shape == sk.alphas_.shape
    assert np.abs(m.alphas_ / sk.alphas_ - 1).max() <= 1e-12
    best = int(np.flatnonzero(sk.alphas_ == sk.alpha_)[0])
    assert m.alpha_ == m.alphas_[best] and abs(m.alpha_ / sk.alpha_ - 1) <= 1e-12
    assert m.mse_path_.shape == sk.mse_path_.shape
    print(f"mse rel {np.abs(m.mse_path_ / sk.mse_path_ - 1).max():.3g}, coef "
          f"{np.abs(m.coef_ - sk.coef_).max() / scale:.3g}")
    assert np.abs(m.mse_path_ / sk.mse_path_ - 1).max() <= 1e-9
    assert m.coef_.shape == sk.coef_.shape and np.shape(m.intercept_) == np.shape(sk.intercept_)
    assert np.abs(m.coef_ - sk.coef_).max() <= bar * scale
    assert abs(m.intercept_ - sk.intercept_) <= bar * scale
    assert m.n_iter_ == sk.n_iter_
    want = X @ m.coef_ + m.intercept_
    pred = m.predict(X)
    assert pred.shape == want.shape
    assert np.abs(pred - want).max() <= 1e-12 * (1 + np.abs(want).max())


@pytest.mark.gpu
@pytest.mark.parametrize("n,p,K", CV_CASES)
@pytest.mark.parametrize("frame", [False, True])
def test_lassocv_dropin_matches_sklearn(n, p, K, frame):
    import pandas as pd
    import afm
    X, y = _cv_data(n, p)
    Xin = pd.DataFrame(X, columns=[f"f{i}" for i in range(p)]) if frame else X
    yin = pd.Series(y, name="target") if frame else y
    for tol in (1e-4, 1e-10):
        m = afm.LassoCV(n_alphas=N_ALPHAS, eps=1e-3, cv=K, tol=tol, max_iter=MAX_ITER)
        m.fit(Xin, yin)
        _check_cv(m, _sk_cv(n, p, K, tol), X, tol)
    if frame:
        assert list(m.feature_names_in_) == list(Xin.columns)


@pytest.mark.gpu
def test_lassocv_single_time_ordered_split():
    import afm
    n, p, K = CV_CASES[1]
    X, y = _cv_data(n, p)
    m = afm.LassoCV(n_alphas=N_ALPHAS, cv=[_time_split(n)], tol=1e-4, max_iter=MAX_ITER).fit(X, y)
    _check_cv(m, _sk_cv(n, p, K, 1e-4, single_split=True), X, 1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("n,p,K", CV_CASES)
def test_lasso_path_dropin_matches_sklearn(n, p, K):
    import pandas as pd
    import sklearn.linear_model as sk
    import afm
    X, y = _cv_data(n, p)
    Xc, yc = X - X.mean(0), y - y.mean()
    for tol, bar in ((1e-4, 1e-6), (1e-12, 1e-9)):
        ra, rc, rg = sk.lasso_path(Xc, yc, eps=1e-3, n_alphas=N_ALPHAS, tol=tol,
                                   max_iter=MAX_ITER)
        a, c, g = afm.lasso_path(pd.DataFrame(X), pd.Series(y), eps=1e-3, n_alphas=N_ALPHAS,
                                 tol=tol, max_iter=MAX_ITER)
        assert a.shape == ra.shape and c.shape == rc.shape and g.shape == rg.shape
        assert np.abs(a / ra - 1).max() <= 1e-12
        assert np.abs(c - rc).max() <= bar * np.abs(rc).max()
    a2, c2, _ = afm.lasso_path(X, y, alphas=ra[::-1][:5], tol=1e-12, max_iter=MAX_ITER)
    assert np.array_equal(a2, np.sort(ra[::-1][:5])[::-1]) and c2.shape == (p, 5)
    with pytest.raises(ValueError):
        afm.lasso_path(X, y, alphas=[0.1, -0.1])


# ---- GPU: the pipeline --------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipeline_lasso_cv():
    import torch
    import afm
    import oracle
    from afm import _lib
    from afm.factors import TARGET
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.synthetic import make_panel
    split = dict(train_end="2001-06-29", valid_end="2001-12-31", window=120)
    grid = afm.PanelGrid.from_panel(make_panel(300, 700, seed=11, tradable_p=0.9))
    pipe = Pipeline(grid, PipelineConfig(**split))
    pipe.step()
    torch.cuda.synchronize()
    first = [t.cpu().numpy().tobytes() for t in (pipe.lasso_beta, pipe.pool_g, pipe.pred)]
    res = pipe.lasso_cv(n_alphas=8)
    p, sp, T, lda = pipe.p, pipe.sp, pipe.T, pipe.lda_r
    assert res["alphas"].shape == (8,) and res["coefs"].shape == (8, p + 1)
    # the path: the oracle chain on the engine's own train Gram
    Gtr = pipe._cv_gram[0].cpu().numpy()
    n, Q, q, yy = oracle.centered_moments(Gtr)
    assert np.abs(res["alphas"] / geom_alphas(np.abs(q).max() / n, 8) - 1).max() <= 1e-12
    c = pipe.cfg
    W, inf = oracle_chain(Q, q, yy, res["alphas"] * n, max_iter=c.max_iter, tol=c.lasso_tol)
    assert res["coefs"][:, 1:].tobytes() == W.tobytes()
    assert res["n_iter"].tolist() == inf[:, 2].astype(int).tolist()
    assert np.array_equal(res["dual_gap"], inf[:, 0] / n)
    # row counts: rows of the range's dates with a zrows bit and a finite target
    rows = afm.unpack_bits(pipe.zrows, T).cpu().numpy()
    tgt = pipe.out[TARGET].cpu().numpy()
    rows &= np.isfinite(tgt)
    assert res["n_train"] == rows[:sp.tr1].sum() == n
    assert res["n_valid"] == rows[sp.v0:sp.v1].sum() > 0
    # scores: predictions of afm_zpredict_f64 on the valid dates against the target plane
    L, P = _lib.lib(), _lib.ptr
    h = pipe.ctx.bind_stream()
    vr = rows[sp.v0:sp.v1]
    yv = tgt[sp.v0:sp.v1][vr]
    for i in (0, 4, 7):
        pred = torch.full((T, lda), float("nan"), dtype=torch.float64, device="cuda")
        beta = torch.from_numpy(res["coefs"][i].copy()).cuda()
        _lib.check(L.afm_zpredict_f64(h, P(pipe.out), T * lda, lda, sp.v0, sp.v1 - sp.v0,
                                      P(pipe.feat), p, P(pipe.zs), P(beta), P(pipe.zrows),
                                      P(pred)))
        pv = pred.cpu().numpy()[sp.v0:sp.v1][vr]
        mse = ((yv - pv) ** 2).mean()
        print(i, res["mse_valid"][i] / mse - 1, res["ic_valid"][i])
        assert abs(res["mse_valid"][i] - mse) <= 1e-10 * mse
        if not res["coefs"][i, 1:].any():
            assert np.isnan(res["ic_valid"][i])
        elif np.ptp(pv) > 1e-6 * np.abs(pv).max():
            assert abs(res["ic_valid"][i] - np.corrcoef(pv, yv)[0, 1]) <= 1e-10
        else:
            # alpha_max itself can leave a weight of a few ulps: the row-form predictions are
            # then constant to rounding and np.corrcoef of them has no digits to compare
            assert i == 0 and abs(res["ic_valid"][i]) <= 1
    assert res["best"] == int(np.argmin(res["mse_valid"]))
    assert res["alpha_"] == res["alphas"][res["best"]]
    # a second step after lasso_cv(): the first step's results, byte for byte
    pipe.step()
    torch.cuda.synchronize()
    again = [t.cpu().numpy().tobytes() for t in (pipe.lasso_beta, pipe.pool_g, pipe.pred)]
    assert again == first
    # the refit: a fresh pipeline's fit at alpha_
    fresh = Pipeline(grid, PipelineConfig(**split, alpha=res["alpha_"]))
    fresh.step()
    torch.cuda.synchronize()
    assert res["beta"].tobytes() == fresh.lasso_beta.cpu().numpy().tobytes()


def test_pipeline_lasso_cv_is_one_gpu_only():
    """The sharded path is out of scope: a rank of a multi-GPU pipeline refuses instead of
    returning the path of its own shard."""
    from types import SimpleNamespace
    from afm.pipeline import Pipeline
    with pytest.raises(NotImplementedError):
        Pipeline.lasso_cv(SimpleNamespace(W=2))
