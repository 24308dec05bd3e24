"""Gradient-boosted regression trees on the device (csrc/gbt.hip, include/afm_gbt.h) -- the
reference's XGBoost models (KKT:481-576, 644-662) without leaving the GPU.

Squared error, histogram splits on at most 256 quantile bins per column, level-wise growth.  The
gradients are quantised to integers each round, so a fit is reproducible to the last bit whatever
the work split; ``tests/gbt_ref.py`` restates the algorithm in numpy.

``GBTParams`` names the hyper-parameters, ``fit_device`` runs a fit on device buffers (what
``Pipeline.gbt_fit`` calls on the resident panel), ``GBTModel`` holds the fitted trees on the host
and ``GBTRegressor`` is the frame / array interface.

Attribution (csrc/gbt_shap.hip, include/afm_gbt_shap.h): a fit also stores the ``cover`` of every
node (the sum of the weights of the training rows that reach it), ``contribs_dense`` /
``GBTRegressor.predict(pred_contribs=True)`` give the exact path-dependent TreeSHAP contributions
of every column to every prediction (XGBoost's layout: ``[n][p + 1]``, the bias last) and
``Pipeline.gbt_contribs`` their per-date means on the resident panel; ``tests/gbt_shap_ref.py``
restates them in numpy.

Out of scope: the multi-GPU pipeline; objectives other than squared error; column / row
subsampling; missing values (the rows are the z-score rows: every value is finite); early
stopping inside the fit (``best_round`` names the round of highest validation IC afterwards, and
``predict(n_trees=...)`` uses a prefix of the trees).
"""
from __future__ import annotations

import operator
from dataclasses import asdict, dataclass

import numpy as np

from . import _lib

MAX_DEPTH, MAX_BIN, MAX_COLS, MAX_WEIGHT = 6, 256, 256, 4095
LEAF, ABSENT = -1, -2
MOMENTS = ["n", "sum_f", "sum_y", "sum_ff", "sum_yy", "sum_fy"]


@dataclass(frozen=True)
class GBTParams:
    """Hyper-parameters of a boosted fit.  ``max_depth``, ``eta`` and ``n_rounds`` default to the
    reference's (KKT:481-487); ``reg_lambda``, ``gamma`` and ``min_child_weight`` to XGBoost's.
    ``base_score`` defaults to 0.0 because the label is a cross-sectional excess return, centred
    on zero by construction; old XGBoost's 0.5 and new XGBoost's label mean are both passable
    values."""
    n_rounds: int = 400
    max_depth: int = 3
    eta: float = 0.025
    reg_lambda: float = 1.0
    gamma: float = 0.0
    min_child_weight: float = 1.0
    max_bin: int = 256
    base_score: float = 0.0

    def __post_init__(self):
        for name, lo, hi in (("n_rounds", 1, 1 << 20), ("max_depth", 1, MAX_DEPTH),
                             ("max_bin", 2, MAX_BIN)):
            v = getattr(self, name)
            try:
                v = operator.index(v)
            except TypeError:
                raise ValueError(f"{name}={getattr(self, name)!r}: expected an integer") from None
            if not lo <= v <= hi:
                raise ValueError(f"{name}={v}: expected {lo}..{hi}")
            object.__setattr__(self, name, v)
        for name, lo in (("eta", None), ("reg_lambda", 0.0), ("gamma", 0.0),
                         ("min_child_weight", 1.0), ("base_score", None)):
            v = getattr(self, name)
            if isinstance(v, (str, bytes, bool)) or not isinstance(v, (int, float, np.number)):
                raise ValueError(f"{name}={v!r}: expected a number")
            v = float(v)
            if not np.isfinite(v) or (lo is not None and v < lo):
                raise ValueError(f"{name}={v}: expected a finite number"
                                 + (f" >= {lo}" if lo is not None else ""))
            object.__setattr__(self, name, v)

    @property
    def n_nodes(self) -> int:
        return 2 ** (self.max_depth + 1) - 1


def _check_params(params) -> GBTParams:
    if params is None:
        return GBTParams()
    if not isinstance(params, GBTParams):
        raise TypeError(f"params: expected a GBTParams, got {type(params).__name__}")
    return params


def metrics(evals: np.ndarray):
    """rmse and the reference's pearson_ic (KKT:490-493) from moments [...][6]."""
    n, sf, sy, sff, syy, sfy = np.moveaxis(np.asarray(evals, dtype=np.float64), -1, 0)
    with np.errstate(all="ignore"):
        rmse = np.sqrt((sff - 2 * sfy + syy) / n)
        ic = (n * sfy - sf * sy) / np.sqrt((n * sff - sf * sf) * (n * syy - sy * sy))
    return rmse, ic


def evals_frame(evals: np.ndarray):
    """evals [n_rounds][2][6] -> a frame per round: train_rmse, train_ic, valid_rmse, valid_ic,
    n_train, n_valid (the valid columns NaN where no row has weight 0)."""
    import pandas as pd
    rmse, ic = metrics(evals)
    return pd.DataFrame({"train_rmse": rmse[:, 0], "train_ic": ic[:, 0], "valid_rmse": rmse[:, 1],
                         "valid_ic": ic[:, 1], "n_train": evals[:, 0, 0].astype(np.int64),
                         "n_valid": evals[:, 1, 0].astype(np.int64)},
                        index=pd.RangeIndex(1, len(evals) + 1, name="round"))


def device_cuts(base, cols_t, w, *, T, lda, col_stride, zs, rows_t, rows_a, n, max_bin):
    """The cuts of every column (plumbing: afm_gbt_values_f64, torch.sort, an index,
    unique_consecutive) -> (cuts [p][max_bin - 1] zero padded, ncuts [p] int32) on the device."""
    import torch
    dev = base.device
    ctx = _lib.Context.get(dev.index)
    p = int(cols_t.numel())
    train = torch.nonzero(w > 0).view(-1)
    m = int(train.numel())
    if m == 0:
        raise ValueError("gbt: no row has a positive weight")
    pos = (torch.arange(1, max_bin, device=dev, dtype=torch.int64) * m) // max_bin
    vals = torch.empty(n, dtype=torch.float64, device=dev)
    cuts = torch.zeros((p, max_bin - 1), dtype=torch.float64, device=dev)
    ncuts = torch.zeros(p, dtype=torch.int32, device=dev)
    for k in range(p):
        ctx.call("afm_gbt_values_f64", base, col_stride, T, lda, cols_t, k, zs, rows_t, rows_a, n,
                 vals)
        s = torch.sort(vals[train]).values
        c = torch.unique_consecutive(s[pos]) + 0.0               # -0.0 -> 0.0
        cuts[k, :c.numel()] = c
        ncuts[k] = c.numel()
    return cuts, ncuts


def fit_device(base, cols, y, w, params: GBTParams, *, T: int, lda: int, n: int, zs=None,
               rows_t=None, rows_a=None, col_stride=None, bufs=None) -> dict:
    """A boosted fit on device buffers, on the current stream.  Row i < n is the cell (rows_t[i],
    rows_a[i]) of the planes base + cols[k] * col_stride ([T][lda]; None: date 0 / asset i),
    z-scored with ``zs`` where given; ``y`` float64 [n], ``w`` int32 [n] (0 = evaluated only).
    Returns device tensors: cuts, ncuts, bins [p][n_pad], feat / bin / thr / val [n_rounds][nn],
    F [n], evals [n_rounds][2][6] and cover [n_rounds][nn] int64 (the sum of w over the rows that
    reach each node: the fit's H).  Nothing synchronises the host after the cuts."""
    import torch
    params = _check_params(params)
    dev = base.device
    ctx = _lib.Context.get(dev.index)
    ctx.bind_stream()
    cols_t = (cols.to(device=dev, dtype=torch.int32).contiguous() if isinstance(cols, torch.Tensor)
              else torch.as_tensor(np.ascontiguousarray(cols, dtype=np.int32), device=dev))
    p = int(cols_t.numel())
    if not 1 <= p <= MAX_COLS:
        raise ValueError(f"gbt: expected 1..{MAX_COLS} columns, got {p}")
    if col_stride is None:
        col_stride = T * lda
    B, D, R, nn = params.max_bin, params.max_depth, params.n_rounds, params.n_nodes
    n_pad = (n + 63) // 64 * 64
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    cuts, ncuts = device_cuts(base, cols_t, w, T=T, lda=lda, col_stride=col_stride, zs=zs,
                              rows_t=rows_t, rows_a=rows_a, n=n, max_bin=B)
    bins = torch.empty((p, n_pad), dtype=torch.uint8, device=dev)
    ctx.call("afm_gbt_bin_f64", base, col_stride, T, lda, cols_t, p, zs, rows_t, rows_a, n, n_pad,
             cuts, ncuts, B, bins)
    res = {"cuts": cuts, "ncuts": ncuts, "bins": bins,
           "feat": torch.empty((R, nn), **i32), "bin": torch.empty((R, nn), **i32),
           "thr": torch.empty((R, nn), **f64), "val": torch.empty((R, nn), **f64),
           "F": torch.full((n,), params.base_score, **f64),
           "evals": torch.empty((R, 2, 6), **f64)}
    nbytes = ctx.call("afm_gbt_scratch_bytes", n, p, D, B)
    scr = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    ctx.call("afm_gbt_fit_f64", bins, n, n_pad, p, cuts, ncuts, y, w, R, D, B, params.eta,
             params.reg_lambda, params.gamma, params.min_child_weight, res["feat"], res["bin"],
             res["thr"], res["val"], res["F"], res["evals"], scr)
    res["cover"] = torch.empty((R, nn), dtype=torch.int64, device=dev)
    ctx.call("afm_gbt_cover_i64", bins, n, n_pad, p, w, res["feat"], res["bin"], D, R, res["cover"])
    if bufs is not None:
        bufs["gbt_scratch"] = scr
    return res


class GBTModel:
    """A fitted ensemble on the host: the tree arrays ``feat`` / ``bin`` / ``thr`` / ``val``
    [n_rounds][nn] in heap order (``feat`` >= 0: the split column, -1: a leaf, -2: absent),
    ``cuts`` / ``ncuts``, ``params``, ``features`` (column names), ``cover`` (int64 [n_rounds][nn],
    the sum of the training weights that reach each node; None on a model saved without it),
    ``evals`` (a frame per round: rmse and IC of the rows that train and of those only evaluated)
    and ``best_round`` (1-based: the round of highest validation IC, the last round when there is
    no validation row)."""

    def __init__(self, params: GBTParams, features, feat, bin, thr, val, cuts, ncuts, evals_raw,
                 cover=None):
        self.params = params
        self.features = [str(f) for f in features]
        self.feat, self.bin = np.asarray(feat, np.int32), np.asarray(bin, np.int32)
        self.thr, self.val = np.asarray(thr, np.float64), np.asarray(val, np.float64)
        self.cuts, self.ncuts = np.asarray(cuts, np.float64), np.asarray(ncuts, np.int32)
        self.evals_raw = np.asarray(evals_raw, np.float64)
        self.cover = None if cover is None else np.asarray(cover, np.int64)
        if self.cover is not None and self.cover.shape != self.feat.shape:
            raise ValueError(f"cover: expected shape {self.feat.shape}, got {self.cover.shape}")
        self.evals = evals_frame(self.evals_raw)
        ic = self.evals["valid_ic"].to_numpy()
        self.best_round = (int(np.nanargmax(ic)) + 1 if np.isfinite(ic).any()
                           else len(self.feat))
        self._dev = None
        self._dev_cover = None

    @classmethod
    def from_device(cls, res: dict, params: GBTParams, features) -> "GBTModel":
        h = {k: res[k].cpu().numpy() for k in ("feat", "bin", "thr", "val", "cuts", "ncuts",
                                               "evals")}
        cover = res["cover"].cpu().numpy() if "cover" in res else None
        return cls(params, features, h["feat"], h["bin"], h["thr"], h["val"], h["cuts"],
                   h["ncuts"], h["evals"], cover=cover)

    @property
    def n_trees(self) -> int:
        return len(self.feat)

    def device_trees(self, device):
        """(feat, thr, val) on ``device`` (cached)."""
        import torch
        if self._dev is None or self._dev[0] != device:
            self._dev = (device, tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                                       for a in (self.feat, self.thr, self.val)))
        return self._dev[1]

    def device_cover(self, device):
        """``cover`` on ``device`` (cached); ValueError when the model has none."""
        import torch
        if self.cover is None:
            raise ValueError("the model has no cover (saved before the fit stored it): refit it")
        if self._dev_cover is None or self._dev_cover[0] != device:
            self._dev_cover = (device,
                               torch.from_numpy(np.ascontiguousarray(self.cover)).to(device))
        return self._dev_cover[1]

    def importance(self, kind: str = "weight") -> np.ndarray:
        """Per column: 'weight' = the number of splits on it (XGBoost's get_score default, the
        count the reference ranks by, KKT:548); 'gain' = the mean decrease of the leaf values'
        spread, |val[left] - val[right]| averaged over its splits (a proxy on the stored arrays:
        the split gains themselves are not kept); 'cover' / 'total_cover' = the mean / the sum of
        the cover of its splits (XGBoost's names; ValueError on a model without ``cover``)."""
        p = len(self.features)
        split = self.feat >= 0
        cnt = np.bincount(self.feat[split], minlength=p).astype(np.float64)
        if kind == "weight":
            return cnt
        if kind in ("cover", "total_cover"):
            if self.cover is None:
                raise ValueError(f"kind={kind!r}: the model has no cover")
            tot = np.bincount(self.feat[split], weights=self.cover[split].astype(np.float64),
                              minlength=p)
            if kind == "total_cover":
                return tot
            with np.errstate(all="ignore"):
                return np.where(cnt > 0, tot / cnt, 0.0)
        if kind != "gain":
            raise ValueError(f"kind={kind!r}: expected 'weight', 'gain', 'cover' or "
                             f"'total_cover'")
        r, v = np.nonzero(split)
        d = np.abs(self.val[r, 2 * v + 1] - self.val[r, 2 * v + 2])
        tot = np.bincount(self.feat[split], weights=d, minlength=p)
        with np.errstate(all="ignore"):
            return np.where(cnt > 0, tot / cnt, 0.0)

    def top_features(self, k: int = 10) -> list:
        """The ``k`` most-split columns, most-split first, ties by column order; columns never
        split on are left out (KKT:548-554)."""
        cnt = self.importance("weight")
        order = np.argsort(-cnt, kind="stable")
        return [self.features[j] for j in order[:k] if cnt[j] > 0]

    def save(self, path):
        extra = {} if self.cover is None else {"cover": self.cover}
        np.savez(path, **extra, feat=self.feat, bin=self.bin, thr=self.thr, val=self.val,
                 cuts=self.cuts, ncuts=self.ncuts, evals=self.evals_raw,
                 features=np.asarray(self.features, dtype=str),
                 params_names=np.asarray(list(asdict(self.params)), dtype=str),
                 params_values=np.asarray(list(asdict(self.params).values()), dtype=np.float64))

    @classmethod
    def load(cls, path) -> "GBTModel":
        with np.load(path, allow_pickle=False) as z:
            kw = dict(zip(z["params_names"].tolist(), z["params_values"].tolist()))
            for name in ("n_rounds", "max_depth", "max_bin"):
                kw[name] = int(kw[name])
            return cls(GBTParams(**kw), z["features"].tolist(), z["feat"], z["bin"], z["thr"],
                       z["val"], z["cuts"], z["ncuts"], z["evals"],
                       cover=z["cover"] if "cover" in z.files else None)


def _host_matrix(X):
    """-> (host float64 [n][p], names or None); non-finite input is rejected here."""
    import torch
    names = None
    if hasattr(X, "columns"):
        names = [str(c) for c in X.columns]
        X = X.to_numpy(dtype=np.float64)
    if isinstance(X, torch.Tensor):
        X = X.detach().cpu().numpy()
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if X.ndim != 2 or X.shape[0] < 1:
        raise ValueError(f"X: expected a non-empty 2-D design, got shape {X.shape}")
    if not np.isfinite(X).all():
        raise ValueError("X holds NaN or inf: the boosted trees take finite values only")
    return X, names


def _host_vector(y, n, what):
    import torch
    if hasattr(y, "to_numpy"):
        y = y.to_numpy()
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if len(y) != n:
        raise ValueError(f"{what}: expected {n} values, got {len(y)}")
    if not np.isfinite(y).all():
        raise ValueError(f"{what} holds NaN or inf")
    return y


def _dense_planes(X, dev):
    """host [n][p] -> device planes [p][1][n_pad] (column-major, zero padded)."""
    import torch
    n, p = X.shape
    n_pad = (n + 63) // 64 * 64
    base = torch.zeros((p, 1, n_pad), dtype=torch.float64, device=dev)
    base[:, 0, :n] = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    return base, n_pad


class GBTRegressor:
    """``GBTRegressor(**params).fit(X, y, eval_set=None, sample_weight=None)`` -- frames or arrays
    in, like ``afm.Lasso``.  ``eval_set``: ``(X_valid, y_valid)`` or a one-element list of it, as
    XGBoost takes it: rows that are scored every round (``model_.evals``) and never train.
    ``sample_weight``: integers 0..4095 (2 = the row enters twice; 0 = evaluated only).  After the
    fit: ``model_`` (a ``GBTModel``), ``feature_importances_`` (split counts normalised to 1),
    ``best_round_``, ``n_features_in_``, ``feature_names_in_``."""

    def __init__(self, **params):
        self.params = GBTParams(**params)

    def fit(self, X, y, eval_set=None, sample_weight=None):
        import torch
        Xh, names = _host_matrix(X)
        n_tr, p = Xh.shape
        if p > MAX_COLS:
            raise ValueError(f"X has {p} columns: at most {MAX_COLS}")
        yh = _host_vector(y, n_tr, "y")
        if sample_weight is None:
            wh = np.ones(n_tr, dtype=np.int32)
        else:
            sw = _host_vector(sample_weight, n_tr, "sample_weight")
            if (sw != np.rint(sw)).any() or (sw < 0).any() or (sw > MAX_WEIGHT).any():
                raise ValueError(f"sample_weight: expected integers 0..{MAX_WEIGHT}")
            wh = sw.astype(np.int32)
        if eval_set is not None:
            if isinstance(eval_set, list):
                if len(eval_set) != 1:
                    raise ValueError("eval_set: expected one (X, y) pair")
                eval_set = eval_set[0]
            Xv, _ = _host_matrix(eval_set[0])
            if Xv.shape[1] != p:
                raise ValueError(f"eval_set has {Xv.shape[1]} columns, X has {p}")
            yv = _host_vector(eval_set[1], len(Xv), "eval_set y")
            Xh, yh = np.concatenate([Xh, Xv]), np.concatenate([yh, yv])
            wh = np.concatenate([wh, np.zeros(len(Xv), dtype=np.int32)])
        if not (wh > 0).any():
            raise ValueError("no row has a positive weight")
        dev = torch.device("cuda", torch.cuda.current_device())
        _lib.Context.get(dev.index)
        n = len(yh)
        base, n_pad = _dense_planes(Xh, dev)
        res = fit_device(base, np.arange(p, dtype=np.int32), torch.from_numpy(yh).to(dev),
                         torch.from_numpy(wh).to(dev), self.params, T=1, lda=n_pad, n=n)
        feats = names if names is not None else [f"f{j}" for j in range(p)]
        self.model_ = GBTModel.from_device(res, self.params, feats)
        self.train_prediction_ = res["F"][:n_tr].cpu().numpy()
        self.n_features_in_ = p
        if names is not None:
            self.feature_names_in_ = np.asarray(names, dtype=object)
        self.best_round_ = self.model_.best_round
        return self

    @property
    def feature_importances_(self) -> np.ndarray:
        cnt = self.model_.importance("weight")
        return cnt / cnt.sum() if cnt.sum() > 0 else cnt

    def predict(self, X, n_trees=None, pred_contribs=False):
        """The prediction [n]; ``pred_contribs=True``: the TreeSHAP contributions [n][p + 1], the
        bias last (``contribs_dense``)."""
        if pred_contribs:
            return contribs_dense(self.model_, X, n_trees)
        return predict_dense(self.model_, X, n_trees)


def _n_trees(model: GBTModel, n_trees) -> int:
    if n_trees is None:
        return model.n_trees
    n_trees = operator.index(n_trees)
    if not 0 <= n_trees <= model.n_trees:
        raise ValueError(f"n_trees={n_trees}: expected 0..{model.n_trees}")
    return n_trees


def predict_dense(model: GBTModel, X, n_trees=None) -> np.ndarray:
    """The first ``n_trees`` trees (default: all) walked over the rows of X -> host [n]."""
    import torch
    Xh, _ = _host_matrix(X)
    n, p = Xh.shape
    if p != len(model.features):
        raise ValueError(f"X has {p} features, model was fit with {len(model.features)}")
    dev = torch.device("cuda", torch.cuda.current_device())
    base, lda = _dense_planes(Xh, dev)
    bits = torch.zeros((1, lda), dtype=torch.int64, device=dev)
    bits[0, :n] = 1
    pred = torch.empty((1, lda), dtype=torch.float64, device=dev)
    feat, thr, val = model.device_trees(dev)
    cols = torch.arange(p, dtype=torch.int32, device=dev)
    _lib.run("afm_gbt_predict_f64", base, lda, lda, 0, 1, cols, p, None, feat, thr, val,
             model.params.max_depth, _n_trees(model, n_trees), model.params.base_score, bits, pred)
    return pred[0, :n].cpu().numpy()


def check_cover(model: GBTModel, n_trees=None):
    """What the contributions need of ``model.cover``, checked on the host: it is there, every
    present node of the first ``n_trees`` trees has cover >= 1, and a split's cover is the sum of
    its children's.  ValueError otherwise."""
    if model.cover is None:
        raise ValueError("the model has no cover (saved before the fit stored it): the "
                         "contributions need the cover of every node -- refit it")
    R = _n_trees(model, n_trees)
    feat, cover = model.feat[:R], model.cover[:R]
    if (cover[feat != ABSENT] < 1).any():
        raise ValueError("cover: a present node has cover < 1")
    r, v = np.nonzero(feat >= 0)
    if (cover[r, v] != cover[r, 2 * v + 1] + cover[r, 2 * v + 2]).any():
        raise ValueError("cover: a split's cover is not the sum of its children's")


def shap_device(ctx, model: GBTModel, n_trees, base, col_stride, lda, t0, nt, cols, p, zs, bits,
                *, contrib: bool, agg: bool) -> dict:
    """afm_gbt_shap_f64 on device buffers, on the context's stream: ``contrib`` [nt][p+1][lda]
    and / or ``agg`` [nt][p+1][2] with ``cnt`` [nt] (include/afm_gbt_shap.h)."""
    import torch
    dev = base.device
    feat, thr, val = model.device_trees(dev)
    cover = model.device_cover(dev)
    D = model.params.max_depth
    nbytes = ctx.call("afm_gbt_shap_scratch_bytes", lda, nt, p, D, n_trees)
    scr = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    out = {"contrib": torch.empty((nt, p + 1, lda), dtype=torch.float64, device=dev)
           if contrib else None,
           "agg": torch.empty((nt, p + 1, 2), dtype=torch.float64, device=dev) if agg else None,
           "cnt": torch.empty(nt, dtype=torch.int64, device=dev) if agg else None}
    ctx.call("afm_gbt_shap_f64", base, col_stride, lda, t0, nt, cols, p, zs, feat, thr, val, cover,
             D, n_trees, model.params.base_score, bits, scr, out["contrib"], out["agg"],
             out["cnt"])
    return out


def contribs_dense(model: GBTModel, X, n_trees=None) -> np.ndarray:
    """The exact path-dependent TreeSHAP contributions of the first ``n_trees`` trees (default:
    all) on the rows of X -> host [n][p + 1], the bias last (XGBoost's ``pred_contribs``): each
    row sums to the prediction up to rounding."""
    import torch
    Xh, _ = _host_matrix(X)
    n, p = Xh.shape
    if p != len(model.features):
        raise ValueError(f"X has {p} features, model was fit with {len(model.features)}")
    R = _n_trees(model, n_trees)
    check_cover(model, R)
    dev = torch.device("cuda", torch.cuda.current_device())
    base, lda = _dense_planes(Xh, dev)
    bits = torch.zeros((1, lda), dtype=torch.int64, device=dev)
    bits[0, :n] = 1
    cols = torch.arange(p, dtype=torch.int32, device=dev)
    ctx = _lib.Context.get(dev.index)
    ctx.bind_stream()
    out = shap_device(ctx, model, R, base, lda, lda, 0, 1, cols, p, None, bits, contrib=True,
                      agg=False)
    return np.ascontiguousarray(out["contrib"][0, :, :n].T.cpu().numpy())
