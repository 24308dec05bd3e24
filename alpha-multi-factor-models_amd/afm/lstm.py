"""Ensembles of stacked LSTMs on the device (csrc/lstm.hip, include/afm_lstm.h) -- the reference's
LSTM(100, return_sequences) -> LSTM(100) -> Dense(1) (KKT:709-769) and its 128 -> 64 variant
(KKT:772-789) fitted with Adam on MSE without shuffling, ``len(seeds)`` of them side by side.

A row is a sequence ``[T][d]``.  ``T = p, d = 1`` is the reference's layout (the feature axis fed
in as time, its ``np.reshape``); ``T = lookback, d = p`` is a window of the last dates of a
security (``Pipeline.lstm_fit(lookback=L)``).

The fit is a deterministic function of the rows, the initial weights and the Adam recurrences;
``include/afm_lstm.h`` pins it and ``tests/lstm_ref.py`` restates it in numpy.  There is no random
number generator on the device: ``lstm_init`` draws Keras's default initial weights on the host.

``LSTMParams`` names the hyper-parameters, ``fit_device`` / ``grad_device`` / ``forward_device``
run on device buffers, ``LSTMModel`` holds the fitted ensemble on the host and ``LSTMRegressor`` is
the frame / array interface.

Out of scope: dropout (Keras's mask stream cannot be reproduced; at prediction it is the
identity), shuffling, other optimisers, more than two recurrent layers, GRU and bidirectional
layers, the multi-GPU pipeline, fp32 or lower-precision training.
"""
from __future__ import annotations

import ctypes
import operator
from dataclasses import dataclass

import numpy as np

from . import _lib
from .gbt import MOMENTS, _host_vector, metrics  # noqa: F401
from .mlp import _member, _number

MAX_STEPS, MAX_INPUTS, MAX_HIDDEN = 256, 64, 128
MAX_MODELS, MAX_BATCH, MAX_EPOCHS = 64, 1024, 4096


def param_count(d: int, h1: int, h2: int) -> int:
    return (d + h1) * 4 * h1 + 4 * h1 + (h1 + h2) * 4 * h2 + 4 * h2 + h2 + 1


@dataclass(frozen=True)
class LSTMParams:
    """Hyper-parameters of an ensemble fit; the defaults are the reference's first network
    (KKT:719-747) with Keras's Adam constants.  ``seeds``: one member per seed (``lstm_init``);
    ``lr``: a scalar, or one learning rate per seed.  ``restore_best``: the fitted weights of a
    member are those of its epoch of lowest validation rmse (ModelCheckpoint(save_best_only))
    instead of the last epoch's."""
    hidden: tuple = (100, 100)
    lr: object = 1e-3
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
        if len(hidden) != 2 or any(h < 4 or h > MAX_HIDDEN or h % 4 for h in hidden):
            raise ValueError(f"hidden={self.hidden!r}: expected two multiples of 4 in "
                             f"4..{MAX_HIDDEN}")
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


def _check_params(params) -> LSTMParams:
    if params is None:
        return LSTMParams()
    if not isinstance(params, LSTMParams):
        raise TypeError(f"params: expected a LSTMParams, got {type(params).__name__}")
    return params


def _check_shape(T, d):
    if not 1 <= T <= MAX_STEPS:
        raise ValueError(f"lstm: expected 1..{MAX_STEPS} steps, got {T}")
    if not 1 <= d <= MAX_INPUTS:
        raise ValueError(f"lstm: expected 1..{MAX_INPUTS} inputs per step, got {d}")


def lstm_init(d: int, hidden, seed: int) -> np.ndarray:
    """Keras's default initial parameters of one network as the flat ``theta`` of afm_lstm.h,
    drawn in the ``theta`` order from ``np.random.default_rng(seed)``: per layer the input kernel
    Glorot uniform in (-l, l), l = sqrt(6 / (fan_in + 4 H)); the recurrent kernel [H][4 H] with
    orthonormal rows (QR of a (4 H, H) normal matrix, the signs fixed by diag(R), transposed); the
    biases zero, the forget block 1.0 (unit_forget_bias); the dense head Glorot uniform, its bias
    zero."""
    h1, h2 = hidden
    rng = np.random.default_rng(seed)
    parts = []
    for din, H in ((d, h1), (h1, h2)):
        lim = np.sqrt(6.0 / (din + 4 * H))
        parts.append(rng.uniform(-lim, lim, size=din * 4 * H))
        q, r = np.linalg.qr(rng.standard_normal((4 * H, H)))
        q = q * np.sign(np.diag(r))
        parts.append(np.ascontiguousarray(q.T).ravel())
        b = np.zeros(4 * H)
        b[H:2 * H] = 1.0
        parts.append(b)
    lim = np.sqrt(6.0 / (h2 + 1))
    parts += [rng.uniform(-lim, lim, size=h2), np.zeros(1)]
    return np.concatenate(parts)


def _design(X, y=None):
    """(T, d, n_pad) of device planes X [T][d][n_pad] (and y [n_pad])."""
    if X.dim() != 3 or (y is not None and (y.dim() != 1 or X.shape[2] != y.shape[0])):
        raise ValueError(f"lstm: expected X [T][d][n_pad] and y [n_pad], got {tuple(X.shape)}"
                         + ("" if y is None else f" and {tuple(y.shape)}"))
    T, d, n_pad = (int(v) for v in X.shape)
    _check_shape(T, d)
    return T, d, n_pad


def _scratch(ctx, dev, T, d, h1, h2, M, batch):
    import torch
    nbytes = ctx.call("afm_lstm_scratch_bytes", T, d, h1, h2, M, batch)
    free = torch.cuda.mem_get_info(dev)[0]
    if nbytes > free:
        raise ValueError(f"lstm: the scratch of this fit takes {nbytes} bytes (T={T}, "
                         f"hidden=({h1}, {h2}), members={M}, batch={batch}); the device has "
                         f"{free} free")
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)


def fit_device(X, y, n_train: int, n_eval: int, params: LSTMParams, theta0=None, bufs=None) -> dict:
    """An ensemble fit on device buffers, on the current stream.  ``X`` float64 [T][d][n_pad] (one
    plane per (step, input), n_pad a multiple of 64), ``y`` float64 [n_pad]; the rows [0, n_train)
    train in that order, the rows [n_train, n_train + n_eval) are scored at the end of every epoch.
    ``theta0`` [M][P]: the initial parameters (default: ``lstm_init`` of every seed).  Returns
    device tensors: theta [M][P], evals [M][epochs][2][6], snaps [M][epochs][P].  Nothing
    synchronises the host."""
    import torch
    params = _check_params(params)
    dev = X.device
    ctx = _lib.Context.get(dev.index)
    ctx.bind_stream()
    T, d, n_pad = _design(X, y)
    h1, h2 = params.hidden
    M, E, P = params.n_members, params.epochs, param_count(d, h1, h2)
    if theta0 is None:
        theta0 = np.stack([lstm_init(d, params.hidden, s) for s in params.seeds])
    if isinstance(theta0, torch.Tensor):
        theta = theta0.to(device=dev, dtype=torch.float64).clone().contiguous()
    else:
        theta = torch.from_numpy(np.ascontiguousarray(theta0, dtype=np.float64)).to(dev)
    if tuple(theta.shape) != (M, P):
        raise ValueError(f"theta0: expected shape {(M, P)}, got {tuple(theta.shape)}")
    f64 = dict(dtype=torch.float64, device=dev)
    res = {"theta": theta, "evals": torch.zeros((M, E, 2, 6), **f64),
           "snaps": torch.empty((M, E, P), **f64)}
    scr = _scratch(ctx, dev, T, d, h1, h2, M, params.batch_size)
    lr = (ctypes.c_double * M)(*params.lrs.tolist())
    ctx.call("afm_lstm_fit_f64", X, y, n_pad, n_train, n_eval, T, d, h1, h2, M, theta, lr,
             params.beta1, params.beta2, params.eps, params.batch_size, E, res["evals"],
             res["snaps"], scr)
    if bufs is not None:
        bufs["lstm_scratch"] = scr
    return res


def grad_device(X, y, theta, hidden, i0: int, nb: int):
    """(grad [M][P], F [M][n_pad]) of the one batch [i0, i0 + nb) for every model of theta [M][P]
    (device tensors, the current stream): the gradient of the batch's mean squared error from the
    kernels the fit runs, and the batch's predictions (NaN in the other cells)."""
    import torch
    T, d, n_pad = _design(X, y)
    M = int(theta.shape[0])
    ctx = _lib.Context.get(X.device.index)
    ctx.bind_stream()
    grad = torch.zeros_like(theta)
    F = torch.full((M, n_pad), float("nan"), dtype=torch.float64, device=X.device)
    scr = _scratch(ctx, X.device, T, d, hidden[0], hidden[1], M, nb)
    ctx.call("afm_lstm_grad_f64", X, y, n_pad, i0, nb, T, d, hidden[0], hidden[1], M, theta, grad,
             F, scr)
    return grad, F


def forward_device(X, theta, hidden, i0: int = 0, n=None, out=None):
    """out[m][i] = F_m(x_i) for the rows [i0, i0 + n) of the planes X [T][d][n_pad] and every model
    of theta [M][P] (device tensors, the current stream); the other cells of ``out`` [M][n_pad]
    keep their values (NaN in a fresh one)."""
    import torch
    T, d, n_pad = _design(X)
    M = int(theta.shape[0])
    if n is None:
        n = n_pad - i0
    if out is None:
        out = torch.full((M, n_pad), float("nan"), dtype=torch.float64, device=X.device)
    ctx = _lib.Context.get(X.device.index)
    ctx.bind_stream()
    ctx.call("afm_lstm_forward_f64", X, n_pad, i0, n, T, d, hidden[0], hidden[1], M, theta, out)
    return out


class LSTMModel:
    """A fitted ensemble on the host: ``theta`` [M][P] (one flat parameter vector per member, the
    order of afm_lstm.h), ``params``, ``features`` (the column names), ``lookback`` (None: every
    feature is one step, ``T = len(features), d = 1``; L: ``T = L, d = len(features)``), ``evals``
    [M][epochs][2][6], ``snaps`` [M][epochs][P] (or None) and ``best_epoch`` [M] (1-based: the
    epoch of lowest validation rmse, the last epoch when there is no eval row).  With
    ``params.restore_best`` ``theta`` is the snapshot of ``best_epoch``."""

    def __init__(self, params: LSTMParams, features, theta, evals, snaps=None, lookback=None):
        self.params = params
        self.features = [str(f) for f in features]
        self.lookback = None if lookback is None else operator.index(lookback)
        if self.lookback is not None and not 1 <= self.lookback <= MAX_STEPS:
            raise ValueError(f"lookback={lookback}: expected 1..{MAX_STEPS}")
        self.evals = np.asarray(evals, np.float64)
        self.snaps = None if snaps is None else np.asarray(snaps, np.float64)
        rmse = metrics(self.evals)[0][:, :, 1]                               # [M][epochs]
        E = self.evals.shape[1]
        self.best_epoch = np.asarray([int(np.nanargmin(r)) + 1 if np.isfinite(r).any() else E
                                      for r in rmse], dtype=np.int64)
        theta = np.array(theta, dtype=np.float64)
        want = (params.n_members, param_count(self.d, *params.hidden))
        if theta.shape != want:
            raise ValueError(f"theta: expected shape {want}, got {theta.shape}")
        if params.restore_best and self.snaps is not None:
            for m, e in enumerate(self.best_epoch):
                theta[m] = self.snaps[m, e - 1]
        self.theta = theta
        self._dev = None

    @property
    def T(self) -> int:
        return len(self.features) if self.lookback is None else self.lookback

    @property
    def d(self) -> int:
        return 1 if self.lookback is None else len(self.features)

    @classmethod
    def from_device(cls, res: dict, params: LSTMParams, features, lookback=None) -> "LSTMModel":
        return cls(params, features, res["theta"].cpu().numpy(), res["evals"].cpu().numpy(),
                   res["snaps"].cpu().numpy() if res.get("snaps") is not None else None, lookback)

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
        """Views into ``theta[member]``: K1 [d + h1][4 h1], b1, K2 [h1 + h2][4 h2], b2, w [h2], b3
        [1] (the column blocks of K and b in the gate order i, f, g, o)."""
        d, (h1, h2) = self.d, self.params.hidden
        t, out, o = self.theta[member], {}, 0
        for name, shape in (("K1", (d + h1, 4 * h1)), ("b1", (4 * h1,)),
                            ("K2", (h1 + h2, 4 * h2)), ("b2", (4 * h2,)), ("w", (h2,)),
                            ("b3", (1,))):
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
                 ints=np.asarray([prm.epochs, prm.batch_size, int(prm.restore_best),
                                  0 if self.lookback is None else self.lookback], np.int64),
                 floats=np.asarray([prm.beta1, prm.beta2, prm.eps], np.float64))

    @classmethod
    def load(cls, path) -> "LSTMModel":
        with np.load(path, allow_pickle=False) as z:
            lr = z["lr"].tolist()
            prm = LSTMParams(hidden=tuple(z["hidden"].tolist()),
                             lr=lr[0] if bool(z["lr_scalar"]) else tuple(lr),
                             epochs=int(z["ints"][0]), batch_size=int(z["ints"][1]),
                             beta1=float(z["floats"][0]), beta2=float(z["floats"][1]),
                             eps=float(z["floats"][2]), seeds=tuple(z["seeds"].tolist()),
                             restore_best=bool(z["ints"][2]))
            snaps = z["snaps"] if z["snaps"].ndim == 3 else None
            return cls(prm, z["features"].tolist(), z["theta"], z["evals"], snaps,
                       int(z["ints"][3]) or None)


def _host_sequences(X):
    """-> (host float64 [n][T][d], names or None): 3-D input as it is, 2-D input [n][p] read as T =
    p, d = 1 (the reference's np.reshape); non-finite input is rejected here."""
    import torch
    names = None
    if hasattr(X, "columns"):
        names = [str(c) for c in X.columns]
        X = X.to_numpy(dtype=np.float64)
    if isinstance(X, torch.Tensor):
        X = X.detach().cpu().numpy()
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 2:
        X = X[:, :, None]
    if X.ndim != 3 or X.shape[0] < 1:
        raise ValueError(f"X: expected [n][T][d] or [n][p] with n >= 1, got shape {X.shape}")
    if not np.isfinite(X).all():
        raise ValueError("X holds NaN or inf")
    _check_shape(X.shape[1], X.shape[2])
    return X, names


def _sequence_planes(X, dev):
    """host [n][T][d] -> device planes [T][d][n_pad] (zero padded)."""
    import torch
    n, T, d = X.shape
    n_pad = (n + 63) // 64 * 64
    base = torch.zeros((T, d, n_pad), dtype=torch.float64, device=dev)
    base[:, :, :n] = torch.from_numpy(np.ascontiguousarray(X.transpose(1, 2, 0))).to(dev)
    return base, n_pad


def predict_sequences(model: LSTMModel, X, member=None) -> np.ndarray:
    """The prediction of one member, or (default) the mean over the members, on the rows of X ->
    host [n]."""
    import torch
    Xh, _ = _host_sequences(X)
    n = len(Xh)
    if Xh.shape[1:] != (model.T, model.d):
        raise ValueError(f"X has sequences {Xh.shape[1:]}, model was fit with "
                         f"{(model.T, model.d)}")
    member = _member(model, member)
    dev = torch.device("cuda", torch.cuda.current_device())
    base, _ = _sequence_planes(Xh, dev)
    out = forward_device(base, model.device_theta(dev), model.params.hidden, 0, n)
    out = out[member, :n] if member is not None else out[:, :n].mean(dim=0)
    return out.cpu().numpy()


class LSTMRegressor:
    """``LSTMRegressor(**params).fit(X, y, eval_set=None).predict(X, member=None)`` -- like
    ``afm.MLPRegressor``.  ``X``: sequences [n][T][d], or a frame / matrix [n][p] read as T = p, d
    = 1 (KKT:712-716).  ``eval_set``: ``(X_valid, y_valid)`` or a one-element list of it.  After
    the fit: ``model_`` (a ``LSTMModel``), ``best_epoch_``, ``n_features_in_`` and, for a frame,
    ``feature_names_in_``."""

    def __init__(self, **params):
        self.params = LSTMParams(**params)

    def fit(self, X, y, eval_set=None):
        import torch
        flat = np.ndim(X) == 2
        Xh, names = _host_sequences(X)
        n_tr, T, d = Xh.shape
        yh = _host_vector(y, n_tr, "y")
        n_ev = 0
        if eval_set is not None:
            if isinstance(eval_set, list):
                if len(eval_set) != 1:
                    raise ValueError("eval_set: expected one (X, y) pair")
                eval_set = eval_set[0]
            Xv, _ = _host_sequences(eval_set[0])
            if Xv.shape[1:] != (T, d):
                raise ValueError(f"eval_set has sequences {Xv.shape[1:]}, X has {(T, d)}")
            yv = _host_vector(eval_set[1], len(Xv), "eval_set y")
            Xh, yh, n_ev = np.concatenate([Xh, Xv]), np.concatenate([yh, yv]), len(Xv)
        dev = torch.device("cuda", torch.cuda.current_device())
        base, n_pad = _sequence_planes(Xh, dev)
        yd = torch.zeros(n_pad, dtype=torch.float64, device=dev)
        yd[:len(yh)] = torch.from_numpy(yh).to(dev)
        res = fit_device(base, yd, n_tr, n_ev, self.params)
        k = T if flat else d
        feats = names if names is not None else [f"f{j}" for j in range(k)]
        self.model_ = LSTMModel.from_device(res, self.params, feats, None if flat else T)
        self.n_features_in_ = k
        if names is not None:
            self.feature_names_in_ = np.asarray(names, dtype=object)
        self.best_epoch_ = self.model_.best_epoch
        return self

    def predict(self, X, member=None):
        return predict_sequences(self.model_, X, member)
