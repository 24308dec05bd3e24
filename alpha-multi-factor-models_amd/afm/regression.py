"""Cross-sectional / pooled OLS.

* ``LinearRegression`` -- drop-in for the scikit-learn estimator as the reference uses it
  (``KKT Yuliang Jiang.py:582-598``: ``fit(X_df, y_df)``, ``intercept_``, ``coef_``,
  ``predict``).  The Gram of [1, X, y] is built on fp64 MFMA in row segments, the segments are
  combined exactly (Chan), the centered normal equations are solved by a scaled Cholesky.
* ``cross_sectional_ols`` -- the north-star per-date regression (Fama-MacBeth): one Gram per
  date straight from the factor planes, batched solves, FM mean / t-statistics.

All arithmetic runs in csrc/xsreg.hip; torch only holds device buffers.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .factors import COL, N_FACTORS, TARGET

SEG_ROWS = 4096          # rows per Gram segment in long mode (one workgroup each)
DEFAULT_TOL = 1e-10      # relative pivot threshold of the scaled Cholesky


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def xs_gram(base, col_stride: int, seg_stride: int, seg_rows: int, cols, ycol: int, *,
            bits=None, seg0: int = 0, nseg: int, row_limit: int = -1):
    """Raw binding of afm_xs_gram_f64 -> (gram [nseg][p+2][p+2], shift [nseg][p+2])."""
    import torch
    dev = base.device
    cols_t = torch.as_tensor(np.asarray(cols, dtype=np.int32), device=dev)
    p = int(cols_t.numel())
    gram = torch.empty((nseg, p + 2, p + 2), dtype=torch.float64, device=dev)
    shift = torch.empty((nseg, p + 2), dtype=torch.float64, device=dev)
    _lib.run("afm_xs_gram_f64", base, col_stride, seg_stride, seg_rows, row_limit, cols_t, p,
             int(ycol), bits, seg0, nseg, gram, shift)
    return gram, shift


def ols_solve(gram, shift, p: int, tol: float = DEFAULT_TOL):
    """-> (beta [nseg][p+1] (intercept first), nobs [nseg], rank [nseg])."""
    import torch
    nseg = gram.shape[0]
    dev = gram.device
    beta = torch.empty((nseg, p + 1), dtype=torch.float64, device=dev)
    nobs = torch.empty(nseg, dtype=torch.float64, device=dev)
    rank = torch.empty(nseg, dtype=torch.int32, device=dev)
    _lib.run("afm_ols_solve_f64", gram, shift, p, nseg, tol, beta, nobs, rank)
    return beta, nobs, rank


def pool_moments(gram, shift, p: int):
    """Exact combination of per-segment moments -> (gram [1][p+2][p+2], shift [1][p+2])."""
    import torch
    dev = gram.device
    g = torch.empty((1, p + 2, p + 2), dtype=torch.float64, device=dev)
    s = torch.empty((1, p + 2), dtype=torch.float64, device=dev)
    _lib.run("afm_pool_moments_f64", gram.contiguous(), shift.contiguous(), p, gram.shape[0], g,
             s)
    return g, s


def fama_macbeth(beta, rank):
    """mean_t beta_t and t-statistics over dates with a solved regression."""
    import torch
    k = beta.shape[1]
    m = torch.empty(k, dtype=torch.float64, device=beta.device)
    t = torch.empty(k, dtype=torch.float64, device=beta.device)
    _lib.run("afm_fama_macbeth_f64", beta, rank, beta.shape[0], k, m, t)
    return m, t


def predict_grid(planes, lda: int, cols, beta, bits, t0: int, nt: int, per_date: bool = False,
                 out=None, ycheck: int = -1):
    """pred[t][a] = beta0 + sum_j beta_j x_j for grid rows with a mask bit (NaN elsewhere)."""
    import torch
    dev = planes.device
    T = planes.shape[1]
    cols_t = torch.as_tensor(np.asarray(cols, dtype=np.int32), device=dev)
    if out is None:
        out = torch.full((T, lda), float("nan"), dtype=torch.float64, device=dev)
    stride = beta.shape[-1] if per_date else 0
    _lib.run("afm_predict_f64", planes, T * lda, lda, t0, nt, cols_t, int(cols_t.numel()),
             beta.contiguous(), stride, bits, int(ycheck), out)
    return out


def cross_sectional_ols(planes, nanfree, lda: int, cols, ycol: int = TARGET, t0: int = 0,
                        nt: int | None = None, A: int | None = None, tol: float = DEFAULT_TOL):
    """Per-date OLS of ``ycol`` on ``cols`` (plane indices of the factor panel) over the rows
    that survive dropna (``nanfree`` bits and finite values).  Returns a dict with the per-date
    ``gram``/``shift`` moments, ``beta`` [nt][p+1], ``nobs``, ``rank``, and FM ``fm_mean``,
    ``fm_t``."""
    T = planes.shape[1]
    nt = T - t0 if nt is None else nt
    A = lda if A is None else A
    p = len(cols)
    gram, shift = xs_gram(planes, T * lda, lda, A, cols, ycol, bits=nanfree, seg0=t0, nseg=nt)
    beta, nobs, rank = ols_solve(gram, shift, p, tol)
    m, t = fama_macbeth(beta, rank)
    return {"gram": gram, "shift": shift, "beta": beta, "nobs": nobs, "rank": rank,
            "fm_mean": m, "fm_t": t}


class LinearRegression:
    """Drop-in for ``sklearn.linear_model.LinearRegression`` (fit_intercept=True) as used by the
    reference (KKT:582-598).  Accepts DataFrames / arrays on the host or torch CUDA tensors."""

    def __init__(self, fit_intercept: bool = True, tol: float = 1e-14, refine: int = 8):
        if not fit_intercept:
            raise NotImplementedError("only fit_intercept=True (the reference's usage)")
        self.fit_intercept = True
        self.tol = tol
        self.refine = refine

    @staticmethod
    def _as_columns(X):
        """-> (device [p][n] float64 column-major matrix, n, p, feature names or None)."""
        import torch
        names = None
        if hasattr(X, "columns"):
            names = np.asarray([str(c) for c in X.columns], dtype=object)
            X = X.to_numpy(dtype=np.float64)
        if isinstance(X, torch.Tensor):
            Xt = X.to(device=_dev(), dtype=torch.float64)
        else:
            Xt = torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float64))).to(_dev())
        if Xt.ndim == 1:
            Xt = Xt.view(-1, 1)
        n, p = Xt.shape
        return Xt.T.contiguous(), n, p, names

    def fit(self, X, y):
        import torch
        Z, n, p, names, y2d = _design(X, y)
        # Z = [x_1..x_p, y, r]: the residual column r drives the refinement passes
        Z = torch.cat([Z, torch.zeros_like(Z[:1])], dim=0)
        nseg = (n + SEG_ROWS - 1) // SEG_ROWS
        gram, shift = xs_gram(Z, n, SEG_ROWS, SEG_ROWS, list(range(p)), p, nseg=nseg,
                              row_limit=n)
        g, s = pool_moments(gram, shift, p)
        beta, nobs, rank = ols_solve(g, s, p, self.tol)
        # semi-normal equations + iterative refinement (accuracy ~ cond(X) eps instead of
        # cond(X)^2 eps, as scikit-learn's SVD-based lstsq): beta += C^-1 Xc' r
        mean = s[0].contiguous()
        for _ in range(self.refine):
            _lib.run("afm_ols_residual_f64", Z, n, p, p, mean, beta[0], Z[p + 1])
            gr, sr = xs_gram(Z, n, SEG_ROWS, SEG_ROWS, list(range(p)), p + 1, nseg=nseg,
                             row_limit=n)
            g2, s2 = pool_moments(gr, sr, p)
            delta, _, _ = ols_solve(g2, s2, p, self.tol)
            _lib.run("afm_vec_add_f64", p, delta[0, 1:].contiguous(), beta[0, 1:])
        _lib.run("afm_ols_intercept_f64", p, mean, beta[0])
        b = beta[0].cpu().numpy()
        self.rank_ = int(rank[0].item())
        self.n_features_in_ = p
        if names is not None:
            self.feature_names_in_ = names
        if y2d:
            self.coef_ = b[1:].reshape(1, p)
            self.intercept_ = b[:1].copy()
        else:
            self.coef_ = b[1:].copy()
            self.intercept_ = float(b[0])
        self._beta = beta[0].contiguous()
        self._y2d = y2d
        return self

    def predict(self, X):
        pred = _predict(self, X)
        return pred.reshape(-1, 1) if self._y2d else pred


def _predict(model, X):
    """The fitted ``model._beta`` (intercept first) applied to the rows of X -> host [n]."""
    import torch
    Xc, n, p, _ = LinearRegression._as_columns(X)
    if p != model.n_features_in_:
        raise ValueError(f"X has {p} features, model was fit with {model.n_features_in_}")
    lda = (n + 63) // 64 * 64
    base = torch.zeros((p, lda), dtype=torch.float64, device=Xc.device)
    base[:, :n] = Xc
    bits = torch.zeros((1, lda), dtype=torch.int64, device=Xc.device)
    bits[0, :n] = 1
    out = predict_grid(base.view(p, 1, lda), lda, list(range(p)), model._beta, bits, 0, 1)
    return out[0, :n].cpu().numpy()


class ConvergenceWarning(UserWarning):
    """Coordinate descent stopped at max_iter with the duality gap above tolerance (the
    condition under which scikit-learn warns)."""


class Lasso:
    """Drop-in for ``sklearn.linear_model.Lasso`` as the reference uses it
    (``Lasso(alpha=2e-4, max_iter=10000).fit(X_trainvalid, y_trainvalid)``, KKT:605-607).

    Minimises ``(1 / (2 n)) ||y - X w - b||^2 + alpha ||w||_1``.  The design's centered moments
    come from the same device Gram + Chan pooling as ``LinearRegression``; the fit is cyclic
    coordinate descent on them (``afm_lasso_cd_f64``: sklearn's Gram coordinate descent with
    its stopping rule and duality gap).  Results: ``coef_`` (p,), ``intercept_`` (float, or a
    1-element array for a one-column DataFrame / 2-D y, as sklearn), ``n_iter_``,
    ``dual_gap_`` (gap / n), ``n_features_in_``, ``feature_names_in_``."""

    def __init__(self, alpha: float = 1.0, *, fit_intercept: bool = True, precompute=False,
                 copy_X: bool = True, max_iter: int = 1000, tol: float = 1e-4,
                 warm_start: bool = False, positive: bool = False, random_state=None,
                 selection: str = "cyclic"):
        if not fit_intercept:
            raise NotImplementedError("only fit_intercept=True (the reference's usage)")
        if selection != "cyclic":
            raise NotImplementedError("only selection='cyclic' (the reference's usage)")
        if warm_start:
            raise NotImplementedError("warm_start is not supported")
        if alpha < 0 or tol < 0 or max_iter < 1:
            raise ValueError("alpha and tol must be >= 0 and max_iter >= 1")
        self.alpha = float(alpha)
        self.fit_intercept = True
        self.precompute = precompute
        self.copy_X = copy_X
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.warm_start = False
        self.positive = bool(positive)
        self.random_state = random_state
        self.selection = selection

    def fit(self, X, y):
        import warnings

        import torch
        Z, n, p, names, y2d = _design(X, y)
        if self.alpha == 0:
            warnings.warn("With alpha=0 this is ordinary least squares by coordinate descent; "
                          "LinearRegression is the better tool.", UserWarning)
        g, s = _pooled(Z, p)
        w = torch.empty(p, dtype=torch.float64, device=Z.device)
        info = torch.empty(3, dtype=torch.float64, device=Z.device)
        _lib.run("afm_lasso_cd_f64", g, p, self.alpha * n, 0.0, self.max_iter, self.tol,
                 int(self.positive), w, info)
        G = g[0].cpu().numpy()
        mean = s[0].cpu().numpy()[1:] + G[0, 1:] / G[0, 0]
        gap, tol_y, n_iter = info.cpu().numpy()
        self.coef_ = w.cpu().numpy()
        x_off, y_off = mean[:p], mean[p]
        icpt = y_off - np.dot(x_off, self.coef_)                 # sklearn _set_intercept
        self.intercept_ = np.array([icpt]) if y2d else float(icpt)
        self.n_iter_ = int(n_iter)
        self.dual_gap_ = float(gap) / n
        self.n_features_in_ = p
        if names is not None:
            self.feature_names_in_ = names
        if self.n_iter_ >= self.max_iter and not gap < tol_y:
            warnings.warn(f"Objective did not converge. Duality gap: {gap:.3e}, tolerance: "
                          f"{tol_y:.3e}", ConvergenceWarning)
        b = np.concatenate([[icpt], self.coef_])
        self._beta = torch.from_numpy(b).to(Z.device)
        return self

    predict = _predict


# ---- regularisation paths and validation-scored alpha selection ---------------------------------
def lasso_batch(gram, shift, p: int, alphas, *, nprob: int = 1, warm: bool = True,
                max_iter: int = 1000, tol: float = 1e-4, positive: bool = False,
                shared: bool = False):
    """Raw binding of afm_lasso_batch_f64 -> (beta [nprob][nalpha][p+1] (intercept first), info
    [nprob][nalpha][3] = {gap, tol * y'y, n_iter}).  ``gram`` [nprob][p+2][p+2] / ``shift``
    [nprob][p+2] pooled moments (``shared``: one Gram for every problem); ``alphas``: device
    float64 [nalpha], sklearn's alpha.  ``warm``: each problem walks the alphas in the order given,
    every solve started from the previous one's weights; else nprob * nalpha solves from zero."""
    import torch
    dev = gram.device
    nalpha = int(alphas.numel())
    beta = torch.empty((nprob, nalpha, p + 1), dtype=torch.float64, device=dev)
    info = torch.empty((nprob, nalpha, 3), dtype=torch.float64, device=dev)
    gs, ss = (0, 0) if shared else ((p + 2) * (p + 2), p + 2)
    _lib.run("afm_lasso_batch_f64", gram, gs, shift, ss, p, alphas, nalpha, nprob,
             int(bool(warm)), int(max_iter), float(tol), int(bool(positive)), beta, info)
    return beta, info


def gram_score(gram, shift, p: int, beta, *, shared: bool = False):
    """Raw binding of afm_gram_score_f64: models ``beta`` [nprob][nmodel][p+1] scored on the
    datasets whose pooled moments are ``gram`` / ``shift`` -> [nprob][nmodel][4] = {n, mse, r2,
    pooled Pearson IC}, from the moments alone."""
    import torch
    nprob, nmodel = int(beta.shape[0]), int(beta.shape[1])
    out = torch.empty((nprob, nmodel, 4), dtype=torch.float64, device=gram.device)
    gs, ss = (0, 0) if shared else ((p + 2) * (p + 2), p + 2)
    _lib.run("afm_gram_score_f64", gram, gs, shift, ss, p, beta, nmodel, nprob, out)
    return out


def alpha_grid(G, p: int, eps: float = 1e-3, n_alphas: int = 100) -> np.ndarray:
    """scikit-learn 1.7.2's ``_alpha_grid`` (l1_ratio = 1, fit_intercept) from a host copy of the
    pooled Gram ``G`` [p+2][p+2] of [1, x, y]: geomspace(alpha_max, alpha_max * eps, n_alphas)
    with alpha_max = max |Xc' yc| / n."""
    n = G[0, 0]
    q = G[1:p + 1, p + 1] - G[0, 1:p + 1] * G[0, p + 1] / n
    alpha_max = np.sqrt(q ** 2).max() / n
    res = np.finfo(np.float64).resolution
    if alpha_max <= res:
        return np.full(n_alphas, res)
    return np.geomspace(alpha_max, alpha_max * eps, num=n_alphas)


def _given_alphas(alphas) -> np.ndarray:
    a = np.sort(np.asarray(alphas, dtype=np.float64).reshape(-1))[::-1].copy()
    if a.size == 0 or not np.isfinite(a).all() or (a < 0).any():
        raise ValueError("alphas must be a non-empty list of finite values >= 0")
    return a


def _design(X, y, max_features: int | None = None):
    """-> (Z device [p+1][n] = [x_1..x_p, y], n, p, feature names or None, y was 2-D);
    ``max_features``: the Lasso path kernels' limit."""
    import torch
    Xc, n, p, names = LinearRegression._as_columns(X)
    yv = y.to_numpy(dtype=np.float64) if hasattr(y, "to_numpy") else y
    y2d = getattr(yv, "ndim", 1) == 2
    yt = torch.as_tensor(np.asarray(yv, dtype=np.float64) if not isinstance(yv, torch.Tensor)
                         else yv, dtype=torch.float64).to(_dev()).reshape(-1)
    if yt.numel() != n:
        raise ValueError(f"X has {n} rows, y has {yt.numel()}")
    if not (torch.isfinite(Xc).all() and torch.isfinite(yt).all()):
        raise ValueError("Input contains NaN or infinity (as scikit-learn rejects it)")
    if max_features is not None and p > max_features:
        raise ValueError(f"{p} features: the Lasso kernels hold at most {max_features}")
    return torch.cat([Xc, yt.view(1, -1)], dim=0).contiguous(), n, p, names, y2d


def _pooled(Z, p: int):
    """Pooled moments of every row of Z [p+1][n]: segment Grams + Chan pooling."""
    n = Z.shape[1]
    nseg = (n + SEG_ROWS - 1) // SEG_ROWS
    gram, shift = xs_gram(Z, n, SEG_ROWS, SEG_ROWS, list(range(p)), p, nseg=nseg, row_limit=n)
    return pool_moments(gram, shift, p)


def lasso_path(X, y, *, eps: float = 1e-3, n_alphas: int = 100, alphas=None, tol: float = 1e-4,
               max_iter: int = 1000, positive: bool = False):
    """Drop-in for ``sklearn.linear_model.lasso_path`` on raw data: X and y are centered
    internally (no intercept is returned), the grid is scikit-learn's (``alpha_grid``; given
    alphas are sorted descending), and the whole warm-started path is one
    ``afm_lasso_batch_f64`` launch on the pooled Gram.  -> (alphas [n_alphas], coefs
    [p][n_alphas], dual_gaps [n_alphas])."""
    import torch
    if tol < 0 or max_iter < 1:
        raise ValueError("tol must be >= 0 and max_iter >= 1")
    Z, n, p, _, _ = _design(X, y, 110)
    g, s = _pooled(Z, p)
    a = _given_alphas(alphas) if alphas is not None else alpha_grid(g[0].cpu().numpy(), p, eps,
                                                                    n_alphas)
    beta, info = lasso_batch(g, s, p, torch.from_numpy(a).to(Z.device), nprob=1, warm=True,
                             max_iter=max_iter, tol=tol, positive=positive)
    return a, beta[0, :, 1:].T.cpu().numpy().copy(), info[0, :, 0].cpu().numpy() / n


def _kfold(n: int, k: int):
    """scikit-learn's unshuffled KFold: contiguous blocks, the first n % k one row longer."""
    if not 2 <= k <= n:
        raise ValueError(f"cv={k}: need 2 <= cv <= n_samples = {n}")
    sizes = np.full(k, n // k, dtype=np.int64)
    sizes[:n % k] += 1
    idx, out, a = np.arange(n), [], 0
    for sz in sizes:
        out.append((np.concatenate([idx[:a], idx[a + sz:]]), idx[a:a + sz]))
        a += sz
    return out


class LassoCV:
    """Drop-in for ``sklearn.linear_model.LassoCV`` (fit_intercept=True, cyclic selection).

    ``cv``: an int (scikit-learn's unshuffled KFold) or an iterable of (train_idx, test_idx) index
    arrays.  Every fold's train and test moments come from a Gram + Chan pooling over the fold's
    own rows; all folds walk the alpha grid warm-started in one ``afm_lasso_batch_f64`` launch
    and are scored from the test moments in one ``afm_gram_score_f64`` launch; ``alpha_``
    minimises the fold-mean MSE and the refit is a cold ``afm_lasso_fit_f64`` on the full-data
    Gram.  Results: ``alpha_``, ``alphas_``, ``mse_path_`` [n_alphas][n_folds], ``coef_``,
    ``intercept_``, ``n_iter_``, ``dual_gap_``, ``n_features_in_``, ``feature_names_in_``."""

    def __init__(self, *, eps: float = 1e-3, n_alphas: int = 100, alphas=None, cv=5,
                 tol: float = 1e-4, max_iter: int = 1000, positive: bool = False,
                 fit_intercept: bool = True, selection: str = "cyclic"):
        if not fit_intercept:
            raise NotImplementedError("only fit_intercept=True (the reference's usage)")
        if selection != "cyclic":
            raise NotImplementedError("only selection='cyclic' (the reference's usage)")
        if tol < 0 or max_iter < 1 or eps <= 0 or n_alphas < 1:
            raise ValueError("need tol >= 0, max_iter >= 1, eps > 0 and n_alphas >= 1")
        self.eps, self.n_alphas = float(eps), int(n_alphas)
        self.alphas = None if alphas is None else _given_alphas(alphas)
        self.cv = cv
        self.tol, self.max_iter, self.positive = float(tol), int(max_iter), bool(positive)
        self.fit_intercept, self.selection = True, selection

    def fit(self, X, y):
        import warnings

        import torch
        Z, n, p, names, _ = _design(X, y, 110)
        dev = Z.device
        g, s = _pooled(Z, p)
        a = self.alphas if self.alphas is not None else alpha_grid(g[0].cpu().numpy(), p,
                                                                   self.eps, self.n_alphas)
        folds = _kfold(n, self.cv) if isinstance(self.cv, (int, np.integer)) else \
            [(np.asarray(tr, dtype=np.int64), np.asarray(te, dtype=np.int64))
             for tr, te in self.cv]
        if not folds:
            raise ValueError("cv yields no split")
        moments = [[], [], [], []]                      # train gram / shift, test gram / shift
        for tr, te in folds:
            if len(tr) == 0 or len(te) == 0 or min(tr.min(), te.min()) < 0 or \
                    max(tr.max(), te.max()) >= n:
                raise ValueError("cv: empty fold or row index out of range")
            for k, rows in ((0, tr), (2, te)):
                gi, si = _pooled(Z.index_select(1, torch.from_numpy(rows).to(dev)).contiguous(), p)
                moments[k].append(gi)
                moments[k + 1].append(si)
        gtr, str_, gte, ste = (torch.cat(m, dim=0).contiguous() for m in moments)
        K = len(folds)
        beta, _ = lasso_batch(gtr, str_, p, torch.from_numpy(a).to(dev), nprob=K, warm=True,
                              max_iter=self.max_iter, tol=self.tol, positive=self.positive)
        mse = gram_score(gte, ste, p, beta)[:, :, 1].cpu().numpy()       # [K][n_alphas]
        best = int(np.argmin(np.mean(mse, axis=0)))
        self.mse_path_ = np.squeeze(mse.T.copy())          # (a single fold: 1-D, as sklearn)
        self.alphas_ = a.copy()
        self.alpha_ = float(a[best])
        b = torch.empty(p + 1, dtype=torch.float64, device=dev)
        info = torch.empty(3, dtype=torch.float64, device=dev)
        _lib.run("afm_lasso_fit_f64", g, s, p, self.alpha_, self.max_iter, self.tol,
                 int(self.positive), b, info)
        bh = b.cpu().numpy()
        gap, tol_y, n_iter = info.cpu().numpy()
        self.coef_, self.intercept_ = bh[1:].copy(), float(bh[0])
        self.n_iter_, self.dual_gap_ = int(n_iter), float(gap) / n
        self.n_features_in_ = p
        if names is not None:
            self.feature_names_in_ = names
        if self.n_iter_ >= self.max_iter and not gap < tol_y:
            warnings.warn(f"Objective did not converge. Duality gap: {gap:.3e}, tolerance: "
                          f"{tol_y:.3e}", ConvergenceWarning)
        self._beta = b
        return self

    predict = _predict
