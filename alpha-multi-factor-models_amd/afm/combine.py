"""Factor combination: the rolling IC-weighted composite of screened columns -- the step after
the factor screen (csrc/combine.hip, include/afm_combine.h).

On every evaluated date the columns are weighted by what their recent ICs say -- the rolling mean
IC, the rolling ICIR, or the rolling "max-IR" weights inv(Sigma) * mean IC with a shrunk IC
covariance, all taken strictly from the past -- and ``composite[t][a] = sum_k w[t][k] *
x_k[t][a] / sum_k |w[t][k]|`` over the columns present on the row.  In pandas::

    m = ic_df.rolling(window, min_periods).mean().shift(embargo)        # 'ic'
    w = m / ic_df.rolling(window, min_periods).std().shift(embargo)     # 'icir'
    w = w.div(w.abs().sum(axis=1), axis=0)
    composite = (df * w).sum(axis=1) / (df.notna() * w.abs()).sum(axis=1)   # per date

``ICWeights`` names the scheme, ``ic_weights`` and ``combine_grid`` run the two kernels on device
buffers (the factor screen's stage behind its IC: ``screen_grid(..., combine=...)``) and
``combine_factors`` is the frame interface.

Out of scope: the multi-GPU pipeline; feeding the composite to the rebalance as ``expected=``;
weights from anything but the screen's ICs (regression betas, factor returns); an exponentially
weighted window.
"""
from __future__ import annotations

import math
from collections.abc import Mapping
from dataclasses import dataclass

import numpy as np

from . import _lib
from .analyzer import RETURN_TYPES, _buffer, _dev

METHODS = {"equal": 0, "ic": 1, "icir": 2, "maxir": 3}
HORIZON = {"return_1": 1, "return_2": 2, "return_5": 5}
MAX_K = 128
MAX_WINDOW = 1024
INFO = ["n_active", "n_dates", "sum_abs_raw"]


@dataclass(frozen=True)
class ICWeights:
    """The rolling IC weights of a composite.  ``method``: 'equal' (1 / K each), 'ic' (the mean IC
    of the window), 'icir' (mean / sd, ddof = 1) or 'maxir' (inv(A) * mean IC with A = (1 -
    ``shrink``) S + ``shrink`` diag(S), S the covariance of the ICs over the window's dates that
    have every candidate column).  The window of an evaluated date holds the ``window`` evaluated
    dates that end ``embargo`` dates before it; a column needs ``min_periods`` finite ICs in it
    (default ``max(2, window // 2)``).  The weights are scaled to sum \\|w\\| = 1 per date; a
    date without an active column has no weights (NaN).

    ``embargo=None`` means the horizon of ``return_type`` (1, 2 or 5), counted in evaluated dates:
    the IC of a date against ``return_q`` looks ``q`` price rows of each security ahead, so it is
    known only ``q`` dates later.  On a panel whose securities skip dates, ``q`` price rows span
    more than ``q`` dates: there the caller raises ``embargo``."""
    method: str = "icir"
    window: int = 60
    embargo: int | None = None
    min_periods: int | None = None
    shrink: float = 0.5
    return_type: str = "return_1"

    def __post_init__(self):
        if self.method not in METHODS:
            raise ValueError(f"method={self.method!r}: expected one of {sorted(METHODS)}")
        if self.return_type not in HORIZON:
            raise ValueError(f"return_type={self.return_type!r}: expected one of {RETURN_TYPES}")
        window = int(self.window)
        if not 1 <= window <= MAX_WINDOW:
            raise ValueError(f"window={self.window!r}: expected 1..{MAX_WINDOW}")
        embargo = HORIZON[self.return_type] if self.embargo is None else int(self.embargo)
        if embargo < 0:
            raise ValueError(f"embargo={self.embargo!r}: must not be negative")
        minp = max(2, window // 2) if self.min_periods is None else int(self.min_periods)
        if self.min_periods is None and window == 1:
            minp = 1
        if not 1 <= minp <= window or (METHODS[self.method] >= 2 and minp < 2):
            raise ValueError(f"min_periods={minp}: expected 1..window (at least 2 for 'icir' and "
                             "'maxir')")
        shrink = float(self.shrink)
        if not (math.isfinite(shrink) and 0.0 < shrink <= 1.0):
            raise ValueError(f"shrink={self.shrink!r}: expected a number in (0, 1]")
        object.__setattr__(self, "window", window)
        object.__setattr__(self, "embargo", embargo)
        object.__setattr__(self, "min_periods", minp)
        object.__setattr__(self, "shrink", shrink)

    @property
    def code(self) -> int:
        return METHODS[self.method]

    @property
    def q(self) -> int:
        return RETURN_TYPES.index(self.return_type)


def _check_spec(spec) -> ICWeights:
    if not isinstance(spec, ICWeights):
        raise TypeError(f"combine: expected an ICWeights, got {type(spec).__name__}")
    return spec


def ic_weights(ic, spec: ICWeights, bufs=None):
    """``ic`` [nd][K][3] (device, the screen's, evaluated dates ascending) -> device tensors ``w``
    [nd][K] and ``info`` [nd][3] = (n_active, n_dates, sum \\|raw\\|) of ``spec``
    (afm_ic_weights_f64).  ``bufs``: a dict that keeps the buffers between calls (``weights``,
    ``weights_info``)."""
    import torch
    spec = _check_spec(spec)
    nd, K = int(ic.shape[0]), int(ic.shape[1])
    if tuple(ic.shape) != (nd, K, 3):
        raise ValueError(f"ic: expected shape [nd][K][3], got {tuple(ic.shape)}")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{K} columns: a composite takes 1..{MAX_K}")
    dev = ic.device
    ctx = _lib.Context.get(dev.index)
    ctx.bind_stream()
    w = _buffer(bufs, "weights", (nd, K), torch.float64, dev)
    info = _buffer(bufs, "weights_info", (nd, 3), torch.float64, dev)
    ctx.call("afm_ic_weights_f64", ic if nd else None, nd, K, spec.q, spec.code, spec.window,
             spec.embargo, spec.min_periods, spec.shrink, w if nd else None,
             info if nd else None)
    return w, info


def combine_grid(base, cols, rows_idx, nrows, dates_idx, w, *, T: int, lda: int, zs=None,
                 zcols=None, col_stride=None, bufs=None):
    """Device-level composite on grids.  ``base``, ``cols``, ``zs``, ``zcols``, ``col_stride``:
    the planes and values of ``screen_grid``; ``rows_idx`` [T][lda] / ``nrows`` [T] (int32): the
    compacted asset indices of each date's rows; ``dates_idx``: the evaluated dates; ``w``:
    weights [nd][K], or [K] for every date (a tensor or an array; brought to a contiguous float64
    tensor on the device of ``base``).

    Returns device tensors ``out`` [T][lda] -- on the rows of an evaluated date sum w x / sum
    \\|w\\| over the columns whose value is finite and whose weight is finite and not 0 (NaN where
    there is none), NaN on its other cells; the rows of other dates are left as they are (NaN in a
    buffer allocated here) -- and ``cnt`` [T][lda] (int32), the number of columns that counted
    (afm_combine_f64).  ``bufs``: a dict that keeps the buffers (``composite``,
    ``composite_cnt``)."""
    import torch
    dev = base.device
    f64, i32 = torch.float64, torch.int32
    ctx = _lib.Context.get(dev.index)
    ctx.bind_stream()

    def dev_i32(v):
        if isinstance(v, torch.Tensor):
            return v.to(device=dev, dtype=i32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev)

    cols_t = dev_i32(cols)
    K = int(cols_t.numel())
    if not 1 <= K <= MAX_K:
        raise ValueError(f"{K} columns: a composite takes 1..{MAX_K}")
    zc_t = dev_i32(zcols) if zcols is not None else None
    d_t = dev_i32(dates_idx)
    nd = int(d_t.numel())
    if col_stride is None:
        col_stride = T * lda
    if not isinstance(w, torch.Tensor):
        w = torch.as_tensor(np.asarray(w, dtype=np.float64))
    w = w.to(device=dev, dtype=f64).contiguous()
    if tuple(w.shape) == (K,):
        w_stride = 0
    elif tuple(w.shape) == (nd, K):
        w_stride = K
    else:
        raise ValueError(f"w: expected shape ({nd}, {K}) or ({K},), got {tuple(w.shape)}")
    kept = bufs.get("composite") if bufs is not None else None
    out = _buffer(bufs, "composite", (T, lda), f64, dev)
    cnt = _buffer(bufs, "composite_cnt", (T, lda), i32, dev)
    if out is not kept:                                    # allocated here
        out.fill_(float("nan"))
        cnt.zero_()
    ctx.call("afm_combine_f64", base, col_stride, T, lda, cols_t, K, zs, zc_t, d_t, nd, rows_idx,
             nrows, w, w_stride, out, cnt)
    return out, cnt


def screen_composite(call, spec, ic, base, col_stride, cols_t, zs, zc_t, d_t, rows, rows_idx,
                     nrows, corr_method, bufs, rank_bufs=None) -> dict:
    """The combination stage of ``screen_grid``: the weights from the screen's ``ic``, the
    composite over the screen's shared rows, and its own IC and summary as a one-column panel.
    ``rank_bufs``: the dict in which the screen's rank IC left the return ranks of the dates."""
    import torch
    from .analyzer import rank_ic
    T, lda = rows_idx.shape
    dev = ic.device
    nd = int(ic.shape[0])
    w, info = ic_weights(ic, spec, bufs)
    out, cnt = combine_grid(base, cols_t, rows_idx, nrows, d_t, w, T=T, lda=lda, zs=zs,
                            zcols=zc_t, col_stride=col_stride, bufs=bufs)
    cic = _buffer(bufs, "composite_ic", (nd, 1, 3), torch.float64, dev)
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    if corr_method == "spearman":
        rank_ic(call, out, T * lda, one, 1, None, None, d_t, nd, rows, rows_idx, nrows, cic,
                rank_bufs, ranked=rank_bufs is not None)
    else:
        call("afm_screen_ic_f64", out, T * lda, T, lda, one, 1, None, None, d_t, nd, rows,
             rows_idx, nrows, cic)
    cst = _buffer(bufs, "composite_stats", (1, 3, 5), torch.float64, dev)
    scr = _buffer(bufs, "composite_scratch", (1, 3, 2, max(nd, 1)), torch.float64, dev)
    call("afm_screen_summary_f64", cic if nd else scr, nd, 1, one, 0, 0, cst, scr, scr)
    return {"weights": w, "weights_info": info, "composite": out, "composite_cnt": cnt,
            "composite_ic": cic.view(nd, 3), "composite_stats": cst.view(3, 5)}


def _frame_grid(factors_df, cols):
    """The (date, id) frame as device grids: base [K][T][lda], rows_idx, nrows, the scatter
    indices of the frame's rows, the dates."""
    import torch
    from .xsprep import rows_of_mask
    dcol = factors_df.index.get_level_values(0).to_numpy()
    icol = factors_df.index.get_level_values(1).to_numpy()
    dates, t_idx = np.unique(dcol, return_inverse=True)
    ids, a_idx = np.unique(icol, return_inverse=True)
    T, A, K = len(dates), len(ids), len(cols)
    lda = (A + 63) // 64 * 64
    dev = _dev()
    st = torch.from_numpy(t_idx.astype(np.int64)).to(dev)
    sa = torch.from_numpy(a_idx.astype(np.int64)).to(dev)
    base = torch.full((K, T, lda), float("nan"), dtype=torch.float64, device=dev)
    vals = np.ascontiguousarray(factors_df[cols].to_numpy(np.float64).T)
    base[:, st, sa] = torch.from_numpy(vals).to(dev)
    mask = torch.zeros((T, lda), dtype=torch.bool, device=dev)
    mask[st, sa] = True
    rows_idx, nrows = rows_of_mask(mask)
    return base, rows_idx, nrows, st, sa, T, lda


def combine_factors(factors_df, price_data=None, columns=None, weights=ICWeights(), prep=None,
                    groups=None):
    """``combine_factors(factors_df, price_data=None, columns=None, weights=ICWeights(),
    prep=None, groups=None)``: the composite of the columns of ``factors_df`` -- indexed (date,
    id), one column per factor -- as a Series named ``"composite"`` on (date, id), NaN dropped.

    ``weights``: an ``ICWeights`` -- the rolling IC weights against the forward returns of
    ``price_data`` (what ``FactorScreen`` takes); the result is ``FactorScreen(factors_df,
    price_data, columns, prep=prep, groups=groups, combine=weights).run().composite`` -- or a
    mapping name -> static weight.  With a mapping no prices are needed and only the combination
    kernel runs, the weights passed as given for every date: sum w x / sum \\|w\\| over the
    columns present on the row, no normalisation beyond that.  ``prep`` / ``groups``: the per-date
    preprocessing of every column first (``preprocess_factors``)."""
    import pandas as pd
    import torch
    from .xsprep import frame_columns
    if not isinstance(weights, Mapping):
        _check_spec(weights)
        if price_data is None:
            raise ValueError("combine_factors: IC weights need price_data")
        from .screen import FactorScreen
        return FactorScreen(factors_df, price_data, columns=columns, prep=prep, groups=groups,
                            combine=weights).run().composite
    cols = frame_columns(factors_df, columns, groups) if columns is not None else list(weights)
    missing = [c for c in cols if c not in weights or c not in factors_df.columns]
    if missing:
        raise ValueError(f"combine_factors: {missing} lack a weight or are not columns")
    empty = pd.Series(np.zeros(0), index=factors_df.index[:0], name="composite")
    if not len(cols) or not len(factors_df):
        return empty
    if prep is not None:
        from .xsprep import preprocess_factors
        factors_df = preprocess_factors(factors_df, cols, groups, prep)
    base, rows_idx, nrows, st, sa, T, lda = _frame_grid(factors_df, cols)
    w = torch.tensor([float(weights[c]) for c in cols], dtype=torch.float64, device=base.device)
    out, _ = combine_grid(base, np.arange(len(cols)), rows_idx, nrows, np.arange(T), w, T=T,
                          lda=lda)
    got = pd.Series(out[st, sa].cpu().numpy(), index=factors_df.index, name="composite")
    return got.dropna()
