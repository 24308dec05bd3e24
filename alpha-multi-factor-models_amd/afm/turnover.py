"""Factor stability: the rank autocorrelation and the turnover of screened columns -- what a
column costs to trade, next to what the IC says it predicts (csrc/turnover.hip,
include/afm_turnover.h).

For every evaluated date, column and lag -- the date ``lag`` evaluated dates earlier -- three
numbers: the correlation of the column's cross-sectional ranks on the two dates over the
securities ranked on both; the share of the top (bottom) decile layer that was not in it on the
earlier date; and the turnover ``0.5 * sum |w1 - w0|`` of the factor-weighted top-10 book.  In
pandas::

    r = df.groupby('date').rank().unstack()
    rank_autocorr = r.corrwith(r.shift(lag), axis=1)               # per date
    top = layer == 10; top_turnover = (top & ~top.shift(lag)).sum(axis=1) / top.sum(axis=1)

``Turnover`` names the lags, ``turnover_grid`` runs the kernels on device buffers (the factor
screen's stage behind its IC: ``screen_grid(..., turnover=...)``) and ``factor_turnover`` is the
frame interface.

Out of scope: the multi-GPU pipeline; a Spearman re-ranked over the joint set of the two dates
(each date keeps its own ranks); IC decay over horizons other than 1, 2 and 5; cost-adjusted layer
returns; feeding turnover into ``select_factors``.
"""
from __future__ import annotations

import ctypes
import operator
from dataclasses import dataclass

import numpy as np

from . import _lib
from .analyzer import _buffer

MAX_LAGS = 8
COUNTS = ["n_joint", "n_top", "new_top", "n_bot", "new_bot"]
SERIES = ["rank_autocorr", "top_turnover", "bottom_turnover", "port_turnover"]


@dataclass(frozen=True)
class Turnover:
    """The lags of the stability statistics, in evaluated dates: unique ascending integers >= 1,
    at most ``MAX_LAGS`` of them (1 = day over day, 5 = week over week, 21 = month over month)."""
    lags: tuple = (1, 5, 21)

    def __post_init__(self):
        try:
            lags = tuple(operator.index(v) for v in self.lags)
        except TypeError:
            raise ValueError(f"lags={self.lags!r}: expected integers") from None
        if not 1 <= len(lags) <= MAX_LAGS:
            raise ValueError(f"lags={self.lags!r}: expected 1..{MAX_LAGS} lags")
        if lags[0] < 1 or any(b <= a for a, b in zip(lags, lags[1:])):
            raise ValueError(f"lags={self.lags!r}: expected unique ascending integers >= 1")
        object.__setattr__(self, "lags", lags)


def _check_spec(spec) -> Turnover:
    if not isinstance(spec, Turnover):
        raise TypeError(f"turnover: expected a Turnover, got {type(spec).__name__}")
    return spec


def turnover_grid(base, cols, rows_idx, nrows, dates_idx, *, T: int, lda: int, spec: Turnover,
                  zs=None, zcols=None, col_stride=None, bufs=None, prefix: str = "") -> dict:
    """Device-level stability statistics on grids.  ``base``, ``cols``, ``zs``, ``zcols``,
    ``col_stride``: the planes and values of ``screen_grid``; ``rows_idx`` [T][lda] / ``nrows``
    [T] (int32): the compacted asset indices of each date's rows; ``dates_idx``: the evaluated
    dates, ascending (a host array or a tensor) -- position i pairs with position i - lag.

    Returns device tensors ``rank_ac`` [nd][K][L], ``turnover_counts`` [nd][K][L][5] (int32:
    n_joint, n_top, new_top, n_bot, new_bot), ``port_turnover`` [nd][K][L] and ``turnover_stats``
    [K][L][4][2] = (n, mean) of rank_ac, new_top / n_top, new_bot / n_bot and port_turnover over
    their non-NaN dates (afm_screen_turnover_f64, afm_screen_turnover_summary_f64).  The first
    ``lag`` positions of a lag are NaN / 0.  ``bufs``: a dict that keeps the buffers between calls
    (the result's names and ``turnover_scratch``, each with ``prefix`` in front)."""
    import torch
    spec = _check_spec(spec)
    dev = base.device
    f64, i32 = torch.float64, torch.int32
    ctx = _lib.Context.get(dev.index)
    ctx.bind_stream()

    def dev_i32(v):
        if isinstance(v, torch.Tensor):
            return v.to(device=dev, dtype=i32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev)

    d_host = (dates_idx.cpu().numpy() if isinstance(dates_idx, torch.Tensor)
              else np.asarray(dates_idx))
    if d_host.size > 1 and not (np.diff(d_host.astype(np.int64)) > 0).all():
        raise ValueError("turnover: dates_idx must be ascending (a lag counts evaluated dates "
                         "back)")
    cols_t = dev_i32(cols)
    K = int(cols_t.numel())
    zc_t = dev_i32(zcols) if zcols is not None else None
    d_t = dev_i32(dates_idx)
    nd = int(d_t.numel())
    L = len(spec.lags)
    if col_stride is None:
        col_stride = T * lda
    names = [prefix + n for n in ("rank_ac", "turnover_counts", "port_turnover", "turnover_stats")]
    ac = _buffer(bufs, names[0], (nd, K, L), f64, dev)
    cnt = _buffer(bufs, names[1], (nd, K, L, 5), i32, dev)
    pt = _buffer(bufs, names[2], (nd, K, L), f64, dev)
    st = _buffer(bufs, names[3], (K, L, 4, 2), f64, dev)
    if nd:
        nbytes = ctx.call("afm_screen_turnover_scratch_bytes", nd, K, lda)
        scr = _buffer(bufs, prefix + "turnover_scratch", ((nbytes + 7) // 8,), torch.int64, dev)
        lags = (ctypes.c_int32 * L)(*spec.lags)
        ctx.call("afm_screen_turnover_f64", base, col_stride, T, lda, cols_t, K, zs, zc_t, d_t,
                 nd, rows_idx, nrows, lags, L, ac, cnt, pt, scr)
    ctx.call("afm_screen_turnover_summary_f64", ac if nd else None, cnt if nd else None,
             pt if nd else None, nd, K, L, st)
    return dict(zip(names, (ac, cnt, pt, st)))


def turnover_frames(res, dts, names, spec: Turnover, prefix: str = ""):
    """The result of ``turnover_grid`` as frames: ``turnover_df`` (date, factor, lag,
    rank_autocorr, top_turnover, bottom_turnover, port_turnover, n_joint; the rows with position
    >= lag; by date, factor in column order, lag) and the unsorted summary (factor, lag, n and the
    four means; ``n`` counts the dates with a rank autocorrelation)."""
    import pandas as pd
    ac = res[prefix + "rank_ac"].cpu().numpy()                       # [nd][K][L]
    cnt = res[prefix + "turnover_counts"].cpu().numpy()              # [nd][K][L][5]
    pt = res[prefix + "port_turnover"].cpu().numpy()
    st = res[prefix + "turnover_stats"].cpu().numpy()                # [K][L][4][2]
    nd, K, L = ac.shape
    lags = np.asarray(spec.lags, dtype=np.int64)
    names = np.asarray(names, dtype=object)
    keep = (np.arange(nd)[:, None, None] >= lags[None, None, :]) & np.ones((1, K, 1), dtype=bool)
    keep = keep.reshape(-1)
    with np.errstate(all="ignore"):
        top = np.where(cnt[..., 1] > 0, cnt[..., 2] / cnt[..., 1].astype(np.float64), np.nan)
        bot = np.where(cnt[..., 3] > 0, cnt[..., 4] / cnt[..., 3].astype(np.float64), np.nan)
    df = pd.DataFrame({
        "date": np.repeat(np.asarray(dts), K * L)[keep],
        "factor": np.tile(np.repeat(names, L), nd)[keep],
        "lag": np.tile(lags, nd * K)[keep],
        "rank_autocorr": ac.reshape(-1)[keep],
        "top_turnover": top.reshape(-1)[keep],
        "bottom_turnover": bot.reshape(-1)[keep],
        "port_turnover": pt.reshape(-1)[keep],
        "n_joint": cnt[..., 0].reshape(-1)[keep].astype(np.int64)})
    summary = pd.DataFrame({
        "factor": np.repeat(names, L), "lag": np.tile(lags, K),
        "n": st[:, :, 0, 0].reshape(-1).astype(np.int64)})
    for s, name in enumerate(SERIES):
        summary[name] = st[:, :, s, 1].reshape(-1)
    return df, summary


def sort_summary(summary, K: int, L: int):
    """The summary ordered by the mean port_turnover of the smallest lag, ascending; ties keep the
    column order; NaN last; the lags of a factor stay together, ascending."""
    key = summary["port_turnover"].to_numpy().reshape(K, L)[:, 0]
    order = np.argsort(np.where(np.isnan(key), np.inf, key), kind="stable")
    rows = (order[:, None] * L + np.arange(L)[None, :]).reshape(-1)
    return summary.iloc[rows].reset_index(drop=True)


def factor_turnover(factors_df, price_data, columns=None, lags=(1, 5, 21)):
    """``factor_turnover(factors_df, price_data, columns=None, lags=(1, 5, 21))``: the stability
    statistics of the columns of ``factors_df`` -- indexed (date, id), one column per factor --
    over the rows ``FactorScreen`` rates (the frame's rows that have the forward returns of
    ``price_data``): ``(turnover_df, turnover_summary)`` of ``FactorScreen(factors_df, price_data,
    columns, turnover=Turnover(lags)).run()``."""
    from .screen import FactorScreen
    fs = FactorScreen(factors_df, price_data, columns=columns, turnover=Turnover(tuple(lags))).run()
    return fs.turnover_df, fs.turnover_summary
