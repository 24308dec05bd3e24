"""Ensembles of small dense networks on the device (csrc/mlp.hip, include/afm_mlp.h) -- the
reference's Dense(128, relu) -> Dense(32, relu) -> Dense(1) fitted with Adam on MSE without
shuffling (KKT:668-706), ``len(seeds)`` of them side by side, one workgroup per network.

The fit is a deterministic function of the rows, the initial weights and the Adam recurrences;
``include/afm_mlp.h`` pins it and ``tests/mlp_ref.py`` restates it in numpy.  There is no random
number generator on the device: ``glorot_init`` draws Keras's default initial weights on the host.

``MLPParams`` names the hyper-parameters, ``fit_device`` runs a fit on device buffers (what
``Pipeline.mlp_fit`` calls on the resident panel), ``MLPModel`` holds the fitted ensemble on the
host and ``MLPRegressor`` is the frame / array interface.

The reference's stacked LSTMs are ``afm.lstm``.  Out of scope here: dropout, other optimisers,
shuffling; one model over several workgroups; the multi-GPU pipeline; fp32 or lower-precision
training.
"""
from __future__ import annotations

import ctypes
import operator
from dataclasses import dataclass

import numpy as np

from . import _lib
from .gbt import MOMENTS, _host_matrix, _host_vector, metrics  # noqa: F401

MAX_COLS, MAX_HIDDEN, MAX_WIDTH_SUM, MAX_WEIGHTS = 64, 128, 192, 16384
MAX_MODELS, MAX_BATCH, MAX_EPOCHS = 1024, 4096, 4096


def param_count(p: int, h1: int, h2: int) -> int:
    return p * h1 + h1 + h1 * h2 + h2 + h2 + 1


def _number(name, v):
    if isinstance(v, (str, bytes, bool)) or not isinstance(v, (int, float, np.number)):
        raise ValueError(f"{name}={v!r}: expected a number")
    return float(v)


@dataclass(frozen=True)
class MLPParams:
    """Hyper-parameters of an ensemble fit; the defaults are the reference's network (KKT:668-680)
    with Keras's Adam constants.  ``seeds``: one member per seed (``glorot_init``); ``lr``: a
    scalar, or one learning rate per seed.  ``restore_best``: the fitted weights of a member are
    those of its epoch of lowest validation rmse (ModelCheckpoint(save_best_only)) instead of the
    last epoch's."""
    hidden: tuple = (128, 32)
    lr: object = 1e-4
    epochs: int = 10
    batch_size: int = 256
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-7
    seeds: tuple = (2023,)
    restore_best: bool = False

    def __post_init__(self):
        try:
            hidden = tuple(operator.index(h) for h in self.hidden)
        except TypeError:
            raise ValueError(f"hidden={self.hidden!r}: expected two integers") from None
        if len(hidden) != 2 or any(h < 16 or h > MAX_HIDDEN or h % 16 for h in hidden):
            raise ValueError(f"hidden={self.hidden!r}: expected two multiples of 16 in "
                             f"16..{MAX_HIDDEN}")
        if sum(hidden) > MAX_WIDTH_SUM:
            raise ValueError(f"hidden={hidden}: the widths sum to more than {MAX_WIDTH_SUM}")
        object.__setattr__(self, "hidden", hidden)
        for name, hi in (("epochs", MAX_EPOCHS), ("batch_size", MAX_BATCH)):
            v = getattr(self, name)
            try:
                v = operator.index(v)
            except TypeError:
                raise ValueError(f"{name}={getattr(self, name)!r}: expected an integer") from None
            if not 1 <= v <= hi:
                raise ValueError(f"{name}={v}: expected 1..{hi}")
            object.__setattr__(self, name, v)
        try:
            seeds = tuple(operator.index(s) for s in self.seeds)
        except TypeError:
            raise ValueError(f"seeds={self.seeds!r}: expected integers") from None
        if not 1 <= len(seeds) <= MAX_MODELS or any(s < 0 for s in seeds):
            raise ValueError(f"seeds: expected 1..{MAX_MODELS} non-negative integers")
        object.__setattr__(self, "seeds", seeds)
        lr = self.lr
        if isinstance(lr, (list, tuple, np.ndarray)):
            lr = tuple(_number("lr", v) for v in lr)
            if len(lr) != len(seeds):
                raise ValueError(f"lr: expected a scalar or {len(seeds)} values (one per seed)")
        else:
            lr = _number("lr", lr)
        for v in (lr if isinstance(lr, tuple) else (lr,)):
            if not np.isfinite(v) or v <= 0:
                raise ValueError(f"lr={v}: expected a finite number > 0")
        object.__setattr__(self, "lr", lr)
        for name in ("beta1", "beta2", "eps"):
            v = _number(name, getattr(self, name))
            if name == "eps" and (not np.isfinite(v) or v <= 0):
                raise ValueError(f"eps={v}: expected a finite number > 0")
            if name != "eps" and not 0.0 <= v < 1.0:
                raise ValueError(f"{name}={v}: expected a number in [0, 1)")
            object.__setattr__(self, name, v)
        if not isinstance(self.restore_best, (bool, np.bool_)):
            raise ValueError(f"restore_best={self.restore_best!r}: expected a bool")
        object.__setattr__(self, "restore_best", bool(self.restore_best))

    @property
    def n_members(self) -> int:
        return len(self.seeds)

    @property
    def lrs(self) -> np.ndarray:
        """The learning rate of every member."""
        return np.asarray(self.lr if isinstance(self.lr, tuple)
                          else (self.lr,) * len(self.seeds), dtype=np.float64)


def _check_params(params) -> MLPParams:
    if params is None:
        return MLPParams()
    if not isinstance(params, MLPParams):
        raise TypeError(f"params: expected a MLPParams, got {type(params).__name__}")
    return params


def _check_shape(p, hidden):
    h1, h2 = hidden
    if not 1 <= p <= MAX_COLS:
        raise ValueError(f"mlp: expected 1..{MAX_COLS} columns, got {p}")
    if h1 * ((p + 3) // 4 * 4 + h2) > MAX_WEIGHTS:
        raise ValueError(f"mlp: {p} columns with hidden={hidden} exceed {MAX_WEIGHTS} weights "
                         f"(h1 * (p rounded up to 4 + h2))")


def glorot_init(p: int, hidden, seed: int) -> np.ndarray:
    """Keras's default initial parameters of one network as the flat ``theta`` of afm_mlp.h: each
    weight matrix uniform in (-l, l), l = sqrt(6 / (fan_in + fan_out)), drawn in the ``theta``
    order from ``np.random.default_rng(seed)``; the biases zero."""
    h1, h2 = hidden
    rng = np.random.default_rng(seed)
    parts = []
    for fan_in, fan_out in ((p, h1), (h1, h2), (h2, 1)):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        parts += [rng.uniform(-lim, lim, size=fan_in * fan_out), np.zeros(fan_out)]
    return np.concatenate(parts)


def fit_device(X, y, n_train: int, n_eval: int, params: MLPParams, theta0=None, bufs=None) -> dict:
    """An ensemble fit on device buffers, on the current stream.  ``X`` float64 [p][n_pad] (one
    plane per column, n_pad a multiple of 64), ``y`` float64 [n_pad]; the rows [0, n_train) train
    in that order, the rows [n_train, n_train + n_eval) are scored at the end of every epoch.
    ``theta0`` [M][P]: the initial parameters (default: ``glorot_init`` of every seed).  Returns
    device tensors: theta [M][P], evals [M][epochs][2][6], snaps [M][epochs][P].  Nothing
    synchronises the host."""
    import torch
    params = _check_params(params)
    dev = X.device
    ctx = _lib.Context.get(dev.index)
    ctx.bind_stream()
    if X.dim() != 2 or y.dim() != 1 or X.shape[1] != y.shape[0]:
        raise ValueError(f"mlp: expected X [p][n_pad] and y [n_pad], got {tuple(X.shape)} and "
                         f"{tuple(y.shape)}")
    p, n_pad = int(X.shape[0]), int(X.shape[1])
    _check_shape(p, params.hidden)
    h1, h2 = params.hidden
    M, E, P = params.n_members, params.epochs, param_count(p, h1, h2)
    if theta0 is None:
        theta0 = np.stack([glorot_init(p, params.hidden, s) for s in params.seeds])
    if isinstance(theta0, torch.Tensor):
        theta = theta0.to(device=dev, dtype=torch.float64).clone().contiguous()
    else:
        theta = torch.from_numpy(np.ascontiguousarray(theta0, dtype=np.float64)).to(dev)
    if tuple(theta.shape) != (M, P):
        raise ValueError(f"theta0: expected shape {(M, P)}, got {tuple(theta.shape)}")
    f64 = dict(dtype=torch.float64, device=dev)
    res = {"theta": theta, "evals": torch.zeros((M, E, 2, 6), **f64),
           "snaps": torch.empty((M, E, P), **f64)}
    nbytes = ctx.call("afm_mlp_scratch_bytes", p, h1, h2, M, params.batch_size)
    scr = torch.empty((nbytes + 7) // 8, **f64)
    lr = (ctypes.c_double * M)(*params.lrs.tolist())
    ctx.call("afm_mlp_fit_f64", X, y, n_pad, n_train, n_eval, p, h1, h2, M, theta, lr,
             params.beta1, params.beta2, params.eps, params.batch_size, E, res["evals"],
             res["snaps"], scr)
    if bufs is not None:
        bufs["mlp_scratch"] = scr
    return res


def forward_device(X, theta, hidden, i0: int = 0, n=None, out=None):
    """out[m][i] = f_m(x_i) for the rows [i0, i0 + n) of the planes X [p][n_pad] and every model of
    theta [M][P] (device tensors, the current stream); the other cells of ``out`` [M][n_pad] keep
    their values (NaN in a fresh one)."""
    import torch
    p, n_pad = int(X.shape[0]), int(X.shape[1])
    _check_shape(p, hidden)
    M = int(theta.shape[0])
    if n is None:
        n = n_pad - i0
    if out is None:
        out = torch.full((M, n_pad), float("nan"), dtype=torch.float64, device=X.device)
    ctx = _lib.Context.get(X.device.index)
    ctx.bind_stream()
    ctx.call("afm_mlp_forward_f64", X, n_pad, i0, n, p, hidden[0], hidden[1], M, theta, out)
    return out


class MLPModel:
    """A fitted ensemble on the host: ``theta`` [M][P] (one flat parameter vector per member, the
    order of afm_mlp.h), ``params``, ``features`` (column names), ``evals`` [M][epochs][2][6] (the
    moments of ``afm.gbt.MOMENTS`` of the training rows -- Keras's running ``loss`` -- and of the
    eval rows at the end of every epoch), ``snaps`` [M][epochs][P] (the parameters at the end of
    every epoch, or None) and ``best_epoch`` [M] (1-based: the epoch of lowest validation rmse, the
    last epoch when there is no eval row).  With ``params.restore_best`` ``theta`` is the snapshot
    of ``best_epoch``."""

    def __init__(self, params: MLPParams, features, theta, evals, snaps=None):
        self.params = params
        self.features = [str(f) for f in features]
        self.evals = np.asarray(evals, np.float64)
        self.snaps = None if snaps is None else np.asarray(snaps, np.float64)
        rmse = metrics(self.evals)[0][:, :, 1]                               # [M][epochs]
        E = self.evals.shape[1]
        self.best_epoch = np.asarray([int(np.nanargmin(r)) + 1 if np.isfinite(r).any() else E
                                      for r in rmse], dtype=np.int64)
        theta = np.array(theta, dtype=np.float64)
        p, (h1, h2) = len(self.features), params.hidden
        if theta.shape != (params.n_members, param_count(p, h1, h2)):
            raise ValueError(f"theta: expected shape "
                             f"{(params.n_members, param_count(p, h1, h2))}, got {theta.shape}")
        if params.restore_best and self.snaps is not None:
            for m, e in enumerate(self.best_epoch):
                theta[m] = self.snaps[m, e - 1]
        self.theta = theta
        self._dev = None

    @classmethod
    def from_device(cls, res: dict, params: MLPParams, features) -> "MLPModel":
        return cls(params, features, res["theta"].cpu().numpy(), res["evals"].cpu().numpy(),
                   res["snaps"].cpu().numpy() if res.get("snaps") is not None else None)

    @property
    def n_members(self) -> int:
        return len(self.theta)

    def evals_frame(self, member: int = 0):
        """The per-epoch frame of one member: train_rmse, train_ic, valid_rmse, valid_ic, n_train,
        n_valid (``afm.gbt.metrics`` of the moments; the valid columns NaN without eval rows)."""
        import pandas as pd
        ev = self.evals[member]
        rmse, ic = metrics(ev)
        return pd.DataFrame({"train_rmse": rmse[:, 0], "train_ic": ic[:, 0],
                             "valid_rmse": rmse[:, 1], "valid_ic": ic[:, 1],
                             "n_train": ev[:, 0, 0].astype(np.int64),
                             "n_valid": ev[:, 1, 0].astype(np.int64)},
                            index=pd.RangeIndex(1, len(ev) + 1, name="epoch"))

    def layers(self, member: int = 0) -> dict:
        """Views into ``theta[member]``: W1 [p][h1], b1, W2 [h1][h2], b2, w3 [h2], b3 [1]."""
        p, (h1, h2) = len(self.features), self.params.hidden
        t, out, o = self.theta[member], {}, 0
        for name, shape in (("W1", (p, h1)), ("b1", (h1,)), ("W2", (h1, h2)), ("b2", (h2,)),
                            ("w3", (h2,)), ("b3", (1,))):
            k = int(np.prod(shape))
            out[name] = t[o:o + k].reshape(shape)
            o += k
        return out

    def device_theta(self, device):
        """``theta`` on ``device`` (cached)."""
        import torch
        if self._dev is None or self._dev[0] != device:
            self._dev = (device, torch.from_numpy(np.ascontiguousarray(self.theta)).to(device))
        return self._dev[1]

    def save(self, path):
        prm = self.params
        np.savez(path, theta=self.theta, evals=self.evals,
                 snaps=self.snaps if self.snaps is not None else np.zeros((0,)),
                 features=np.asarray(self.features, dtype=str),
                 hidden=np.asarray(prm.hidden, np.int64), seeds=np.asarray(prm.seeds, np.int64),
                 lr=prm.lrs, lr_scalar=np.asarray(not isinstance(prm.lr, tuple)),
                 ints=np.asarray([prm.epochs, prm.batch_size, int(prm.restore_best)], np.int64),
                 floats=np.asarray([prm.beta1, prm.beta2, prm.eps], np.float64))

    @classmethod
    def load(cls, path) -> "MLPModel":
        with np.load(path, allow_pickle=False) as z:
            lr = z["lr"].tolist()
            prm = MLPParams(hidden=tuple(z["hidden"].tolist()),
                            lr=lr[0] if bool(z["lr_scalar"]) else tuple(lr),
                            epochs=int(z["ints"][0]), batch_size=int(z["ints"][1]),
                            beta1=float(z["floats"][0]), beta2=float(z["floats"][1]),
                            eps=float(z["floats"][2]), seeds=tuple(z["seeds"].tolist()),
                            restore_best=bool(z["ints"][2]))
            snaps = z["snaps"] if z["snaps"].ndim == 3 else None
            return cls(prm, z["features"].tolist(), z["theta"], z["evals"], snaps)


def _member(model: MLPModel, member):
    if member is None:
        return None
    member = operator.index(member)
    if not 0 <= member < model.n_members:
        raise ValueError(f"member={member}: expected 0..{model.n_members - 1}")
    return member


def _dense_planes(X, dev):
    """host [n][p] -> device planes [p][n_pad] (column-major, zero padded)."""
    import torch
    n, p = X.shape
    n_pad = (n + 63) // 64 * 64
    base = torch.zeros((p, n_pad), dtype=torch.float64, device=dev)
    base[:, :n] = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    return base, n_pad


def predict_dense(model: MLPModel, X, member=None) -> np.ndarray:
    """The prediction of one member, or (default) the mean over the members, on the rows of X ->
    host [n]."""
    import torch
    Xh, _ = _host_matrix(X)
    n, p = Xh.shape
    if p != len(model.features):
        raise ValueError(f"X has {p} features, model was fit with {len(model.features)}")
    member = _member(model, member)
    dev = torch.device("cuda", torch.cuda.current_device())
    base, _ = _dense_planes(Xh, dev)
    out = forward_device(base, model.device_theta(dev), model.params.hidden, 0, n)
    out = out[member, :n] if member is not None else out[:, :n].mean(dim=0)
    return out.cpu().numpy()


class MLPRegressor:
    """``MLPRegressor(**params).fit(X, y, eval_set=None).predict(X, member=None)`` -- frames or
    arrays in, like ``afm.GBTRegressor``.  ``eval_set``: ``(X_valid, y_valid)`` or a one-element
    list of it: rows scored at the end of every epoch (``model_.evals``) that never train.  After
    the fit: ``model_`` (a ``MLPModel``), ``best_epoch_``, ``n_features_in_``,
    ``feature_names_in_``."""

    def __init__(self, **params):
        self.params = MLPParams(**params)

    def fit(self, X, y, eval_set=None):
        import torch
        Xh, names = _host_matrix(X)
        n_tr, p = Xh.shape
        _check_shape(p, self.params.hidden)
        yh = _host_vector(y, n_tr, "y")
        n_ev = 0
        if eval_set is not None:
            if isinstance(eval_set, list):
                if len(eval_set) != 1:
                    raise ValueError("eval_set: expected one (X, y) pair")
                eval_set = eval_set[0]
            Xv, _ = _host_matrix(eval_set[0])
            if Xv.shape[1] != p:
                raise ValueError(f"eval_set has {Xv.shape[1]} columns, X has {p}")
            yv = _host_vector(eval_set[1], len(Xv), "eval_set y")
            Xh, yh, n_ev = np.concatenate([Xh, Xv]), np.concatenate([yh, yv]), len(Xv)
        dev = torch.device("cuda", torch.cuda.current_device())
        base, n_pad = _dense_planes(Xh, dev)
        yd = torch.zeros(n_pad, dtype=torch.float64, device=dev)
        yd[:len(yh)] = torch.from_numpy(yh).to(dev)
        res = fit_device(base, yd, n_tr, n_ev, self.params)
        feats = names if names is not None else [f"f{j}" for j in range(p)]
        self.model_ = MLPModel.from_device(res, self.params, feats)
        self.n_features_in_ = p
        if names is not None:
            self.feature_names_in_ = np.asarray(names, dtype=object)
        self.best_epoch_ = self.model_.best_epoch
        return self

    def predict(self, X, member=None):
        return predict_dense(self.model_, X, member)
