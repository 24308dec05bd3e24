"""The multi-factor risk model on the device (csrc/risk.hip, include/afm_risk.h): an EWMA covariance
of the factor returns (the coefficients of the per-date cross-sectional regressions), an EWMA
specific variance per security, the covariance B F B' + D of a book, the risk decomposition of the
books, and the weight solve from that covariance (csrc/portfolio.hip: the exact box QP of the
rebalance entered after its covariance phase).  ``tests/risk_ref.py`` restates the arithmetic in
numpy; the kernels equal it bit for bit.

``RiskParams`` names the parameters, ``fit_device`` runs a fit on device buffers (what
``Pipeline.risk_fit`` calls on the resident panel), ``RiskModel`` holds the device planes,
``book_risk_device`` prices the books of a rebalance result, ``cov_weights`` /
``rebalance_cov_device`` solve from a covariance and ``bias_statistic`` scores the forecasts on the
host.

Out of scope: Newey-West terms and volatility-regime scaling; separate half-lives for volatilities
and correlations; a ``PortfolioManager(risk_model=)`` drop-in; the multi-GPU pipeline; running any
of this inside ``Pipeline.step``.
"""
from __future__ import annotations

import operator
from dataclasses import asdict, dataclass

import numpy as np

from . import _lib
from .portfolio import MAX_BOOK

MAX_FACTORS = 32                     # AFM_RISK_MAX_FACTORS: the intercept and at most 31 columns


@dataclass(frozen=True)
class RiskParams:
    """``half_life`` (dates) of the factor covariance's weights, ``spec_half_life`` of the specific
    variance's (None: ``half_life``), ``min_obs`` used dates (observations of a security) before a
    value is given, ``lag``: the forecast of date t is made from the dates <= t - lag (the label of
    date t is the next day's return: 1 keeps it out of the date's own forecast)."""
    half_life: float = 90.0
    spec_half_life: float | None = None
    min_obs: int = 20
    lag: int = 1

    def __post_init__(self):
        for name, lo in (("min_obs", 1), ("lag", 0)):
            v = getattr(self, name)
            try:
                v = operator.index(v)
            except TypeError:
                raise ValueError(f"{name}={getattr(self, name)!r}: expected an integer") from None
            if not lo <= v < 1 << 31:
                raise ValueError(f"{name}={v}: expected an integer >= {lo}")
            object.__setattr__(self, name, v)
        for name in ("half_life", "spec_half_life"):
            v = getattr(self, name)
            if v is None and name == "spec_half_life":
                continue
            if isinstance(v, (str, bytes, bool)) or not isinstance(v, (int, float, np.number)):
                raise ValueError(f"{name}={v!r}: expected a number")
            v = float(v)
            if not np.isfinite(v) or v <= 0:
                raise ValueError(f"{name}={v}: expected a finite number > 0")
            object.__setattr__(self, name, v)

    @property
    def spec_hl(self) -> float:
        return self.half_life if self.spec_half_life is None else self.spec_half_life


def _check_params(params) -> RiskParams:
    if params is None:
        return RiskParams()
    if not isinstance(params, RiskParams):
        raise TypeError(f"params: expected a RiskParams, got {type(params).__name__}")
    return params


def _check_factors(p: int):
    if not 1 <= p <= MAX_FACTORS - 1:
        raise ValueError(f"{p} exposure columns: the risk model holds the intercept and at most "
                         f"{MAX_FACTORS - 1}")


def model_device(base, cols, ycol: int, bits, beta, rank, params: RiskParams, *, T: int, A: int,
                 lda: int, col_stride: int | None = None) -> dict:
    """The model from given factor returns, on the current stream: ``beta`` [T][p+1] and ``rank``
    [T] (afm_ols_solve_f64's) -> device tensors resid [T][lda], fcov [T][K1][K1], nused [T], spec
    [T][lda], fill [T]."""
    import torch
    dev = base.device
    params = _check_params(params)
    cols_t = torch.as_tensor(np.asarray(cols.cpu() if torch.is_tensor(cols) else cols,
                                        dtype=np.int32), device=dev)
    p = int(cols_t.numel())
    _check_factors(p)
    K1 = p + 1
    cs = T * lda if col_stride is None else int(col_stride)
    ctx = _lib.Context.get(dev.index)
    ctx.bind_stream()
    f64 = dict(dtype=torch.float64, device=dev)
    res = {"resid": torch.empty((T, lda), **f64), "fcov": torch.empty((T, K1, K1), **f64),
           "nused": torch.empty(T, dtype=torch.int32, device=dev),
           "spec": torch.empty((T, lda), **f64), "fill": torch.empty(T, **f64)}
    ctx.call("afm_risk_resid_f64", base, cs, T, A, lda, cols_t, p, int(ycol), beta, rank, bits,
             res["resid"])
    ctx.call("afm_risk_factor_cov_f64", beta, rank, T, p, params.half_life, params.min_obs,
             params.lag, res["fcov"], res["nused"])
    ctx.call("afm_risk_specific_f64", res["resid"], T, A, lda, params.spec_hl, params.min_obs,
             params.lag, res["spec"], res["fill"])
    res.update(beta=beta, rank=rank, cols=cols_t)
    return res


def fit_device(base, cols, ycol: int, bits, params: RiskParams | None = None, *, T: int, A: int,
               lda: int, col_stride: int | None = None, tol: float = 1e-10) -> dict:
    """A fit on device buffers, on the current stream: the per-date OLS of the plane ``ycol`` on the
    planes ``cols`` (base + c * col_stride, [T][lda]) over the rows with a bit set in ``bits``
    (afm_xs_gram_f64 + afm_ols_solve_f64 over all T dates), then ``model_device``.  Returns its
    tensors and nobs [T]."""
    import torch
    from .regression import ols_solve, xs_gram
    params = _check_params(params)
    cols_np = np.asarray(cols.cpu() if torch.is_tensor(cols) else cols, dtype=np.int32)
    _check_factors(len(cols_np))
    cs = T * lda if col_stride is None else int(col_stride)
    gram, shift = xs_gram(base, cs, lda, A, cols_np, int(ycol), bits=bits, seg0=0, nseg=T)
    beta, nobs, rank = ols_solve(gram, shift, len(cols_np), tol)
    res = model_device(base, cols_np, ycol, bits, beta, rank, params, T=T, A=A, lda=lda,
                       col_stride=cs)
    res["nobs"] = nobs
    return res


def book_risk_device(model: dict, base, reb: dict, dates_idx, *, T: int, lda: int, kc: int,
                     col_stride: int | None = None) -> dict:
    """afm_risk_book_f64 on the current stream: the books ``reb`` (k, books, weights of a rebalance)
    at the grid dates ``dates_idx`` priced by ``model`` (``fit_device``'s tensors) -> device tensors
    cov [nd][2][kc][kc] (NaN where nothing is written), risk [nd][3][4], contrib [nd][3][K1],
    status [nd]."""
    import torch
    dev = base.device
    nd = int(dates_idx.numel())
    K1 = int(model["fcov"].shape[1])
    if not 1 <= int(kc) <= MAX_BOOK:
        raise ValueError(f"kc={kc}: expected 1..{MAX_BOOK}")
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"cov": torch.full((nd, 2, kc, kc), float("nan"), **f64),
           "risk": torch.full((nd, 3, 4), float("nan"), **f64),
           "contrib": torch.full((nd, 3, K1), float("nan"), **f64),
           "status": torch.zeros(nd, dtype=torch.int32, device=dev)}
    cs = T * lda if col_stride is None else int(col_stride)
    _lib.run("afm_risk_book_f64", base, cs, T, lda, model["cols"], K1 - 1, dates_idx, nd, reb["k"],
             reb["books"], reb["weights"], model["fcov"], model["spec"], model["fill"], int(kc),
             out["cov"], out["risk"], out["contrib"], out["status"])
    return out


def cov_weights(cov, mu=None, risk_tolerance: float = 0.0, lo: float = 0.0, hi: float = 0.1,
                status: bool = False):
    """One book from a covariance [k][k]: min 1/2 w'Sw - risk_tolerance * mu'w, sum w = 1,
    lo <= w <= hi (``mu`` None: no return term) -> w [k], and with ``status`` the solve's status
    word.  Fed the covariance ``afm.portfolio.mean_variance_weights`` returned, it returns that
    function's weights bit for bit."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    S = torch.as_tensor(np.ascontiguousarray(np.asarray(cov, dtype=np.float64)), device=dev)
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError("cov must be square [k][k]")
    k = int(S.shape[0])
    if not 1 <= k <= MAX_BOOK:
        raise ValueError(f"book of {k}: expected 1..{MAX_BOOK} names")
    m = None
    if mu is not None:
        m = torch.as_tensor(np.ascontiguousarray(np.asarray(mu, dtype=np.float64)), device=dev)
        if tuple(m.shape) != (k,):
            raise ValueError(f"mu must have one value per name ({k})")
    w = torch.empty(k, dtype=torch.float64, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.run("afm_cov_weights_f64", S, k, m, float(risk_tolerance), float(lo), float(hi), w, st)
    return (w.cpu().numpy(), int(st.item())) if status else w.cpu().numpy()


def rebalance_cov_device(reb: dict, cov, dates_idx, close, tmr, *, kc: int, cov_status=None,
                         mu=None, risk_tolerance: float = 0.0, lo: float = 0.0, hi: float = 0.1):
    """afm_rebalance_cov_f64 on the current stream: every (date, side) of ``reb`` solved again from
    ``cov`` [nd][2][kc][kc]; ``reb``'s weights, sums and status are rewritten in place."""
    T, lda = close.shape
    _lib.run("afm_rebalance_cov_f64", T, lda, dates_idx, int(dates_idx.numel()), reb["k"],
             reb["books"], cov, int(kc), cov_status, mu, float(risk_tolerance), float(lo), float(hi),
             close, tmr, reb["weights"], reb["sums"], reb["status"])
    return reb


class RiskModel:
    """A fitted model: the device planes (``fcov`` [T][K1][K1], ``nused`` [T], ``spec`` [T][lda],
    ``fill`` [T], ``beta`` [T][K1], ``rank`` [T], ``cols``; ``resid`` while it is kept) with the
    dates, ids and factor names they are indexed by."""

    _PLANES = ("fcov", "nused", "spec", "fill", "beta", "rank", "cols")

    def __init__(self, params: RiskParams, features, dates, ids, planes: dict):
        self.params = _check_params(params)
        self.features = [str(f) for f in features]
        self.factors = ["intercept"] + self.features
        self.dates, self.ids = np.asarray(dates), np.asarray(ids)
        missing = [k for k in self._PLANES if k not in planes]
        if missing:
            raise ValueError(f"planes: missing {missing}")
        self.planes = dict(planes)
        K1 = len(self.factors)
        if tuple(planes["fcov"].shape) != (len(self.dates), K1, K1):
            raise ValueError("fcov must be [dates][factors][factors]")

    def __getitem__(self, key):
        return self.planes[key]

    @property
    def used(self) -> np.ndarray:
        """[T] bool: the dates whose regression entered the model."""
        beta = self.planes["beta"].cpu().numpy()
        rank = self.planes["rank"].cpu().numpy()
        return (rank == beta.shape[1] - 1) & np.isfinite(beta).all(axis=1)

    @property
    def factor_returns(self):
        """A frame dates x factors: the coefficients of the used dates, NaN on the others."""
        import pandas as pd
        beta = self.planes["beta"].cpu().numpy().copy()
        beta[~self.used] = np.nan
        return pd.DataFrame(beta, index=pd.Index(self.dates, name="date"), columns=self.factors)

    @property
    def factor_vol(self):
        """A frame dates x factors: the square roots of the diagonals of fcov."""
        import pandas as pd
        f = self.planes["fcov"].cpu().numpy()
        with np.errstate(all="ignore"):
            vol = np.sqrt(np.diagonal(f, axis1=1, axis2=2))
        return pd.DataFrame(vol, index=pd.Index(self.dates, name="date"), columns=self.factors)

    def _date_index(self, date) -> int:
        if isinstance(date, (int, np.integer)):
            return int(date)
        hit = np.flatnonzero(self.dates == np.datetime64(date))
        if not len(hit):
            raise KeyError(f"{date!r} is not a date of the model")
        return int(hit[0])

    def factor_corr(self, date):
        """The factor correlation matrix at ``date`` (a date or a grid index) as a frame."""
        import pandas as pd
        f = self.planes["fcov"][self._date_index(date)].cpu().numpy()
        with np.errstate(all="ignore"):
            s = np.sqrt(np.diag(f))
            c = f / (s[:, None] * s[None, :])
        return pd.DataFrame(c, index=self.factors, columns=self.factors)

    def save(self, path):
        arrays = {k: self.planes[k].cpu().numpy() for k in self._PLANES}
        prm = asdict(self.params)
        prm["spec_half_life"] = np.nan if prm["spec_half_life"] is None else prm["spec_half_life"]
        with open(path, "wb") as f:
            np.savez(f, features=np.asarray(self.features, dtype=str), dates=self.dates,
                     ids=self.ids, params=np.asarray([prm[k] for k in sorted(prm)], np.float64),
                     **arrays)

    @classmethod
    def load(cls, path, device=None):
        import torch
        dev = torch.device("cpu") if device is None else device
        with np.load(path, allow_pickle=False) as z:
            keys = sorted(asdict(RiskParams()))
            prm = dict(zip(keys, z["params"].tolist()))
            prm["spec_half_life"] = None if np.isnan(prm["spec_half_life"]) else prm["spec_half_life"]
            prm["min_obs"], prm["lag"] = int(prm["min_obs"]), int(prm["lag"])
            planes = {k: torch.from_numpy(z[k].copy()).to(dev) for k in cls._PLANES}
            return cls(RiskParams(**prm), [str(f) for f in z["features"]], z["dates"], z["ids"],
                       planes)


def bias_statistic(realised, predicted_vol, window: int | None = None):
    """The bias statistic of a volatility forecast, on the host: the standard deviation (ddof 1) of
    the standardised outcomes realised / predicted_vol -- 1 for a forecast that is right on average,
    above 1 where risk was under-forecast.  1-D inputs aligned by position (pairs with a non-finite
    or non-positive forecast are left out); ``window``: a rolling statistic over that many pairs (a
    vector, NaN until the window is full) instead of one number over all of them."""
    r = np.asarray(realised, dtype=np.float64).reshape(-1)
    v = np.asarray(predicted_vol, dtype=np.float64).reshape(-1)
    if r.shape != v.shape:
        raise ValueError("realised and predicted_vol must have the same length")
    ok = np.isfinite(r) & np.isfinite(v) & (v > 0)
    with np.errstate(all="ignore"):
        z = np.where(ok, r / v, np.nan)
    if window is None:
        zz = z[ok]
        return float(np.std(zz, ddof=1)) if len(zz) >= 2 else float("nan")
    window = operator.index(window)
    if window < 2:
        raise ValueError("window must be at least 2")
    out = np.full(len(z), np.nan)
    for i in range(window - 1, len(z)):
        zz = z[i - window + 1:i + 1]
        if np.isfinite(zz).all():
            out[i] = np.std(zz, ddof=1)
    return out
