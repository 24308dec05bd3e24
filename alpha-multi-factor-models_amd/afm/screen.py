"""Factor screening: the per-date IC of many factor columns in one pass.

The reference evaluates single factors on the train split before it fits anything, one column at
a time: ``AlphaSignalAnalyzer(df_train_x[['d11']], 'd11', df_train[['close_price']]).run()``
("KKT Yuliang Jiang.py":465, 472).  All columns of one frame share the rows, the forward returns
and the per-date demeans (KKT:308-320), so ``screen_grid`` prepares those once and evaluates the
IC of every column per date (KKT:342-349) -- Pearson, or with ``corr_method='spearman'`` the rank
IC (the reference's ``corr_method`` attribute, KKT:286) -- its per-year IR (KKT:351-354) and a
whole-sample summary (csrc/screen.hip, csrc/rankic.hip, include/afm_screen.h,
include/afm_rankic.h).  With ``layers=True`` the same pass also gives the other half of the
reference's single-factor evaluation for every column: the decile layered returns, the long-short
spreads and the factor-weighted top-10 backtest (KKT:324-375; csrc/screen_layers.hip,
include/afm_screen_layers.h).  With ``xcorr=True`` it gives what the reference never looks at: how the
columns relate to each other -- the per-date correlation matrix of the screened columns, its mean
over the dates, and ``select_factors``, a greedy "best IR first, drop what is too correlated with
what is kept" choice of columns (csrc/xcorr.hip, include/afm_xcorr.h).  With ``prep=XsPrep(...)``
every column is first winsorised, group-neutralised and standardised across each date
(afm/xsprep.py, csrc/xsprep.hip, include/afm_xsprep.h) and all of the above rate the result.
With ``combine=ICWeights(...)`` the columns are combined into one signal -- on every date weighted
by their rolling ICs of the past -- and the composite is rated next to its ingredients
(afm/combine.py, csrc/combine.hip, include/afm_combine.h).  With ``turnover=Turnover(...)`` it
also says how much every column changes from one date to an earlier one -- the rank
autocorrelation, the turnover of the extreme layers and of the top-10 book -- which is what the
gross returns above have to pay for (afm/turnover.py, csrc/turnover.hip, include/afm_turnover.h).
``FactorScreen`` is the frame interface beside ``AlphaSignalAnalyzer``.

Out of scope: the multi-GPU pipeline.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .analyzer import RETURN_TYPES, _buffer, _dev, check_corr_method, rank_ic
from .grid import pack_bits, unpack_bits

STATS = ["n", "mean", "std", "IR", "t"]


def screen_grid(base, cols, close, price_bits, row_bits, *, A: int, zs=None, zcols=None,
                col_stride=None, dates_idx=None, year=None, bufs=None,
                corr_method="pearson", layers=False, xcorr=False, prep=None, groups=None,
                ngroups=0, combine=None, turnover=None) -> dict:
    """Device-level screen on grids.  ``base``: the panel, plane k of the screen at ``base +
    cols[k] * col_stride`` ([T][lda] each; ``col_stride`` defaults to T * lda); ``close`` [T][lda]
    with ``price_bits`` presence (the price rows of the forward returns); ``row_bits``: the row
    set shared by every column.  ``zs`` (afm_zstats_finalize_f64's {mu, 1/sd} table): the values
    are z = (x - mu) * (1/sd) of row ``zcols[k]`` (default row k), computed where they are read.
    A non-finite value is skipped for its own column only (pandas nancorr).

    One forward-return pass, one ``afm_xs_prepare_f64`` on a plane that is 0.0 on the rows and NaN
    elsewhere (the shared merge / dropna cascade and demeans; A <= 32768 as there), then the IC
    of every (date, column, return) and the summary.  ``dates_idx``: the evaluated dates (default:
    those with rows); ``year`` [T]: calendar years for the per-year IR.  ``corr_method``: 'pearson'
    or 'spearman' (the rank IC: the return ranks of a date are taken once for all columns).

    ``layers=True``: also the backtests of every column on the same preparation and dates, whatever
    ``corr_method`` is -- ``layer_mean`` [nd][K][3][10], ``layer_cnt`` [nd][K][10] (int32),
    ``port`` [nd][K][3], ``cum_layer`` [nd][K][3][10], ``ls`` [nd][K][3][5] and ``cum_port``
    [nd][K][3]: for a column without NaN on the rows what ``evaluate_grid`` gives for it alone,
    bit for bit.  A NaN cell has no rank and is left out for its own column; +-inf cells are
    ranked (pandas ``rank``), unlike in the IC.  The returns stay those demeaned over the shared
    rows.

    ``xcorr=True``: also ``xcorr`` [nd][K][K], the correlation matrix of the K columns on each
    evaluated date over the shared rows (``DataFrame.corr()``: pairwise complete, a non-finite
    cell missing for its own column, NaN under two joint rows or without variance, the diagonal
    exactly 1.0 or NaN), and ``xcorr_stats`` [K][K][3] = (n, mean r, mean \|r\|) of every pair
    over the dates.  On the same preparation and dates as the IC, whatever ``corr_method`` is: the
    factor-to-factor correlation is always Pearson (a Spearman variant is out of scope).

    ``prep`` (an ``afm.xsprep.XsPrep``): every column is first preprocessed across each evaluated
    date -- winsorised, with ``groups`` (int32 [lda] or [T][lda], labels in [0, ``ngroups``))
    group-neutralised, standardised (``afm.xsprep.preprocess_grid``) -- over the rows of
    ``row_bits`` on that date, the cross-section a ``groupby('date').transform`` of the frame sees
    (not only the rows that also have the three forward returns: then the screen of a frame with
    ``prep`` is the screen of the preprocessed frame, bit for bit).  The IC, rank IC, layers and
    correlations then read the preprocessed planes; the result gains ``prep_info`` [nd][K][7] =
    (n, lo, hi, n_lo, n_hi, mean, std) and ``prep_out`` [K][T][lda].  Without ``prep`` nothing is
    launched or allocated for it.

    ``combine`` (an ``afm.combine.ICWeights``): after the IC, ``weights`` [nd][K] and
    ``weights_info`` [nd][3] = (n_active, n_dates, sum \|raw\|) -- the rolling weights of every
    evaluated date from the ICs (those of ``corr_method``) of the dates before it
    (``afm.combine.ic_weights``); ``composite`` [T][lda] and ``composite_cnt`` -- sum w x / sum
    \|w\| over the screen's shared rows (``rows_idx`` / ``nrows``) of what the IC read, ``prep_out``
    when ``prep`` is given, else the raw / z values (``afm.combine.combine_grid``); and
    ``composite_ic`` [nd][3], ``composite_stats`` [3][5]: the IC (or rank IC) and summary kernels
    on the composite as a one-column panel.  ``dates_idx`` must be ascending (the window of a date
    is the positions before it).  Without ``combine`` nothing is launched or allocated for it.

    ``turnover`` (an ``afm.turnover.Turnover``): after the IC, on what the IC read (``prep_out``
    when ``prep`` is given, else the raw / z values) over the screen's shared rows, ``rank_ac``
    [nd][K][L], ``turnover_counts`` [nd][K][L][5] (int32), ``port_turnover`` [nd][K][L] and
    ``turnover_stats`` [K][L][4][2] of every (date, column, lag) against the evaluated date ``lag``
    positions earlier (``afm.turnover.turnover_grid``); with ``combine`` the same of the composite
    as a one-column panel, the names with ``composite_`` in front.  ``dates_idx`` must be
    ascending.  Without ``turnover`` nothing is launched or allocated for it.

    Returns device tensors ``ic`` [nd][K][3], ``stats`` [K][3][5] (n, mean, std, IR, t over the
    non-NaN ICs), ``ir_year`` [nyears][K][3], ``nrows``, ``rows_idx``, and the host arrays
    ``dates_idx``, ``years``, ``year0``.  ``bufs``: a dict that keeps the work buffers between
    calls."""
    import torch
    check_corr_method(corr_method)
    dev = close.device
    T, lda = close.shape
    f64, i32 = torch.float64, torch.int32
    ctx = _lib.Context.get(dev.index)
    ctx.bind_stream()
    call = ctx.call

    def dev_i32(v):
        if isinstance(v, torch.Tensor):
            return v.to(device=dev, dtype=i32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev)

    cols_t = dev_i32(cols)
    K = int(cols_t.numel())
    zc_t = dev_i32(zcols) if zcols is not None else None
    if col_stride is None:
        col_stride = T * lda
    fr = _buffer(bufs, "fr", (3, T, lda), f64, dev)
    call("afm_fwd_returns_f64", T, lda, close, price_bits, fr)
    sig = _buffer(bufs, "sig", (T, lda), f64, dev)
    sig.fill_(float("nan"))
    sig.masked_fill_(unpack_bits(row_bits, T), 0.0)
    scratch = _buffer(bufs, "scratch", (T, lda), f64, dev)
    rows = _buffer(bufs, "rows", (4, T, lda), f64, dev)
    rows_idx = _buffer(bufs, "rows_idx", (T, lda), i32, dev)
    nrows = _buffer(bufs, "nrows", (T,), i32, dev)
    call("afm_xs_prepare_f64", T, A, lda, sig, fr, scratch, rows, rows_idx, nrows)
    if dates_idx is None:
        dates_idx = np.flatnonzero(nrows.cpu().numpy() > 0)
    dates_idx = np.ascontiguousarray(dates_idx, dtype=np.int32)
    nd = len(dates_idx)
    if combine is not None:
        from .combine import _check_spec, screen_composite
        _check_spec(combine)
        if nd > 1 and not (np.diff(dates_idx) > 0).all():
            raise ValueError("combine: dates_idx must be ascending (the rolling window of a date "
                             "is the evaluated dates before it)")
    if turnover is not None:
        from .turnover import _check_spec as _check_turnover, turnover_grid
        _check_turnover(turnover)
        if nd > 1 and not (np.diff(dates_idx) > 0).all():
            raise ValueError("turnover: dates_idx must be ascending (a lag counts evaluated dates "
                             "back)")
    d_t = torch.from_numpy(dates_idx).to(dev)
    prep_res = None
    if prep is not None:
        from .xsprep import preprocess_grid, rows_of_mask
        all_idx, all_n = rows_of_mask(unpack_bits(row_bits, T))
        prep_res = preprocess_grid(base, cols_t, all_idx, all_n, d_t, T=T, lda=lda, prep=prep,
                                   zs=zs, zcols=zc_t, col_stride=col_stride, groups=groups,
                                   ngroups=ngroups, bufs=bufs)
        base, col_stride, zs, zc_t = prep_res["out"], T * lda, None, None
        cols_t = torch.arange(K, dtype=i32, device=dev)
    ic = _buffer(bufs, "ic", (nd, K, 3), f64, dev)
    if corr_method == "spearman":
        # (without a caller's dict the return ranks still live until the composite has used them)
        rank_bufs = bufs if bufs is not None or combine is None else {}
        rank_ic(call, base, col_stride, cols_t, K, zs, zc_t, d_t, nd, rows, rows_idx, nrows, ic,
                rank_bufs)
    else:
        call("afm_screen_ic_f64", base, col_stride, T, lda, cols_t, K, zs, zc_t, d_t, nd, rows,
             rows_idx, nrows, ic)
    if year is not None and nd:
        yr = np.ascontiguousarray(np.asarray(year)[dates_idx], dtype=np.int32)
        y0, ny = int(yr.min()), int(yr.max() - yr.min() + 1)
    else:
        yr, y0, ny = np.zeros(nd, dtype=np.int32), 0, 0
    y_t = torch.from_numpy(yr).to(dev) if nd else torch.zeros(1, dtype=i32, device=dev)
    stats = _buffer(bufs, "stats", (K, 3, 5), f64, dev)
    ir_year = _buffer(bufs, "ir_year", (ny, K, 3), f64, dev)
    sscr = _buffer(bufs, "summary_scratch", (K, 3, 2, max(nd, 1)), f64, dev)
    call("afm_screen_summary_f64", ic if nd else sscr, nd, K, y_t, ny, y0, stats,
         ir_year if ny else sscr, sscr)
    out = {"ic": ic, "stats": stats, "ir_year": ir_year, "nrows": nrows, "rows_idx": rows_idx,
           "dates_idx": dates_idx, "years": yr, "year0": y0}
    if prep_res is not None:
        out.update(prep_info=prep_res["info"], prep_out=prep_res["out"])
    if combine is not None:
        out.update(screen_composite(call, combine, ic, base, col_stride, cols_t, zs, zc_t, d_t,
                                    rows, rows_idx, nrows, corr_method, bufs,
                                    rank_bufs if corr_method == "spearman" else None))
    if turnover is not None:
        out.update(turnover_grid(base, cols_t, rows_idx, nrows, dates_idx, T=T, lda=lda,
                                 spec=turnover, zs=zs, zcols=zc_t, col_stride=col_stride,
                                 bufs=bufs))
        if combine is not None:
            out.update(turnover_grid(out["composite"], np.zeros(1, dtype=np.int32), rows_idx,
                                     nrows, dates_idx, T=T, lda=lda, spec=turnover, bufs=bufs,
                                     prefix="composite_"))
    if layers:
        lm = _buffer(bufs, "layer_mean", (nd, K, 3, 10), f64, dev)
        lc = _buffer(bufs, "layer_cnt", (nd, K, 10), i32, dev)
        port = _buffer(bufs, "port", (nd, K, 3), f64, dev)
        cum_layer = _buffer(bufs, "cum_layer", (nd, K, 3, 10), f64, dev)
        ls = _buffer(bufs, "ls", (nd, K, 3, 5), f64, dev)
        cum_port = _buffer(bufs, "cum_port", (nd, K, 3), f64, dev)
        if nd:
            lscr = _buffer(bufs, "layers_scratch", (nd * K * 40 + K,), f64, dev)
            call("afm_screen_layers_f64", base, col_stride, T, lda, cols_t, K, zs, zc_t, d_t, nd,
                 rows, rows_idx, nrows, lm, lc, port, lscr)
            call("afm_screen_layer_series_f64", nd, K, lm, port, cum_layer, ls, cum_port)
        out.update(layer_mean=lm, layer_cnt=lc, port=port, cum_layer=cum_layer, ls=ls,
                   cum_port=cum_port)
    if xcorr:
        xc = _buffer(bufs, "xcorr", (nd, K, K), f64, dev)
        xs = _buffer(bufs, "xcorr_stats", (K, K, 3), f64, dev)
        if nd:
            call("afm_screen_xcorr_f64", base, col_stride, T, lda, cols_t, K, zs, zc_t, d_t, nd,
                 None, rows_idx, nrows, xc)
        call("afm_screen_xcorr_summary_f64", xc if nd else None, nd, K, xs)
        out.update(xcorr=xc, xcorr_stats=xs)
    return out


def select_factors(names, score, corr_abs, max_corr=0.7, k=None) -> list:
    """Greedy redundancy pruning: walk ``names`` by \|``score``\| descending (stable in the given
    order; a NaN score leaves its name out) and keep a candidate when its ``corr_abs`` with every
    name kept so far is <= ``max_corr`` (a NaN correlation counts as 0); stop at ``k`` names.
    ``score`` [K]: e.g. the whole-sample IR of each name; ``corr_abs`` [K][K]: e.g. the mean
    \|correlation\| over the dates (``FactorScreen.factor_corr_abs``), rows and columns in the
    order of ``names``.  Returns the kept names in the order taken."""
    names = list(names)
    score = np.abs(np.asarray(score, dtype=np.float64).reshape(-1))
    c = np.asarray(corr_abs, dtype=np.float64)
    if score.shape != (len(names),) or c.shape != (len(names), len(names)):
        raise ValueError("select_factors: score [K] and corr_abs [K][K] must match names")
    if k is not None and k < 0:
        raise ValueError("select_factors: k must not be negative")
    c = np.where(np.isnan(c), 0.0, c)
    order = [i for i in np.argsort(-np.where(np.isnan(score), 0.0, score), kind="stable")
             if not np.isnan(score[i])]
    kept = []
    for i in order:
        if k is not None and len(kept) >= k:
            break
        if all(c[i, j] <= max_corr for j in kept):
            kept.append(int(i))
    return [names[i] for i in kept]


LAYER_STATS = ["top_minus_bottom", "monotonic", "top_k"]


def _last_valid(x):
    """x [nd][...] -> [...]: the last non-NaN entry along the dates (NaN where there is none)."""
    ok = ~np.isnan(x)
    if x.shape[0] == 0:
        return np.full(x.shape[1:], np.nan)
    idx = x.shape[0] - 1 - np.argmax(ok[::-1], axis=0)
    v = np.take_along_axis(x, idx[None], axis=0)[0]
    return np.where(ok.any(axis=0), v, np.nan)


def _layer_spearman(final):
    """final [N][10] (NaN: layer absent) -> [N]: the Spearman correlation of the layer number with
    the value over the layers present (average ranks; NaN under two layers or without spread)."""
    import pandas as pd
    have = ~np.isnan(final)
    num = np.where(have, np.arange(1.0, 11.0), np.nan)
    rx = pd.DataFrame(num).rank(axis=1).to_numpy()
    ry = pd.DataFrame(final).rank(axis=1).to_numpy()
    with np.errstate(all="ignore"):
        n = have.sum(axis=1)
        dx = np.where(have, rx - np.nansum(rx, axis=1, keepdims=True) / n[:, None], 0.0)
        dy = np.where(have, ry - np.nansum(ry, axis=1, keepdims=True) / n[:, None], 0.0)
        den = np.sqrt((dx * dx).sum(axis=1) * (dy * dy).sum(axis=1))
        return np.where((n >= 2) & (den > 0), (dx * dy).sum(axis=1) / den, np.nan)


class FactorScreen:
    """``FactorScreen(factors_df, price_data, columns=None, corr_method="pearson",
    layers=False).run()``: the
    IC / IR screen (Pearson, or with 'spearman' the rank IC, as the analyzer's ``corr_method``) of
    every column of ``factors_df`` -- indexed (date, id), one column per factor, e.g. the reference's
    ``df_train_x`` -- against the forward returns of ``price_data`` (what ``AlphaSignalAnalyzer``
    takes: indexed (date, id), a ``close_price`` column).  The row set is the frame's rows; a NaN
    or inf cell is skipped for its own column only.  For a column without NaN the results are
    those of ``AlphaSignalAnalyzer(factors_df[[c]], c, price_data)``'s ``ic_df`` / ``ir_df``.

    After ``run()``: ``ic_df`` (date, factor, Type, IC; NaN ICs dropped; ordered by date, factor
    in column order, Type), ``ir_df`` (year, factor, Type, IR) and ``summary`` (factor, Type, n,
    mean, std, IR, t; by \\|IR\\| descending, ties in column order, NaN last).

    ``layers=True`` adds the analyzer's backtest frames for every column, with a ``factor`` column
    after ``date`` and ordered by date, then factor in column order: ``layered_ret_dfs[rt]``
    (date, factor, layer, rt: the cumulative layer returns, the layers the factor has on any date,
    NaN entries dropped), ``ls_ret_dfs[rt]`` (date, factor, layer, rt: the long-short spreads,
    layer 5 = 10 minus 1 first) and ``port_ret_df`` (date, factor, Type, Returns: the top-10
    returns and their cumulative sums) -- for a column without NaN the rows of
    ``AlphaSignalAnalyzer``'s frames; a NaN cell is left out of its own column's ranks, an inf
    cell is ranked.  And ``layer_summary``: one row per (factor, Type) with ``top_minus_bottom``
    (the last non-NaN cumulative layer 10 minus layer 1), ``monotonic`` (the Spearman correlation
    of the layer number with the final cumulative layer return over the layers present) and
    ``top_k`` (the final cumulative top-10 return), by \\|top_minus_bottom\\| descending as
    ``summary``.

    ``xcorr=True`` adds the relation of the columns to each other: ``factor_corr``,
    ``factor_corr_abs`` and ``factor_corr_n`` (K x K frames, the factor names on both axes: the
    mean and the mean absolute value over the dates of the per-date ``DataFrame.corr()`` of the
    columns, and the number of dates that have it), ``redundant_pairs`` (factor_a, factor_b, mean,
    mean_abs, n: one row per pair a before b with n > 0, by mean_abs descending, ties in column
    order) and ``select(max_corr, k, return_type)``.  Always Pearson.

    ``prep`` (an ``afm.xsprep.XsPrep``) preprocesses every column across each date first --
    winsorise, neutralise by ``groups`` (the sector of every row: a Series on the frame's index, or
    the name of a column of the frame, which is then not a factor), standardise -- over the
    frame's rows of the date: the screen of ``preprocess_factors(factors_df, columns, groups,
    prep)``, bit for bit, without the trip through the host.  It adds ``prep_info_df`` (date,
    factor, n, lo, hi, n_lo, n_hi, mean, std: the rows a column has on the date, its clipping
    bounds and how many rows each clipped, the mean and sd taken out).

    ``combine`` (an ``afm.combine.ICWeights``) combines the columns into one signal, on every date
    weighted by their rolling ICs of the dates before it, and adds ``weights_df`` (date, factor,
    weight; the dates without weights dropped), ``composite`` (a Series named ``"composite"`` on
    (date, id) over the frame's rows that have the three forward returns, NaN dropped) and
    ``composite_summary`` (Type, n, mean, std, IR, t of the composite's own IC: does the
    combination beat its best column?).

    ``turnover`` (an ``afm.turnover.Turnover``) adds how stable every column is against the date
    ``lag`` evaluated dates earlier: ``turnover_df`` (date, factor, lag, rank_autocorr -- the
    correlation of the two dates' ranks over the securities ranked on both --, top_turnover and
    bottom_turnover -- the share of layer 10 / layer 1 that was not in it on the earlier date --,
    port_turnover -- 0.5 sum \\|w1 - w0\\| of the factor-weighted top-10 book --, n_joint; the rows
    with a date ``lag`` positions back; by date, factor in column order, lag) and
    ``turnover_summary`` (factor, lag, n, and the means of the four over their non-NaN dates; ``n``
    counts the dates with a rank autocorrelation; by the mean port_turnover of the smallest lag
    ascending, ties in column order, NaN last, the lags of a factor together).  With
    ``layers=True`` and lag 1 among the lags, ``turnover_summary`` gains ``breakeven_cost`` on the
    lag-1 rows (NaN on the others): the mean of the column's non-NaN top-10 ``return_1`` divided
    by its mean lag-1 port_turnover, the ``trading_cost_rate`` at which the daily rebalanced
    top-10 book nets zero (KKT:887-889).  With ``combine``, ``composite_turnover_summary`` (lag, n
    and the four means of the composite)."""

    def __init__(self, factors_df, price_data, columns=None, corr_method="pearson",
                 layers=False, xcorr=False, prep=None, groups=None, combine=None, turnover=None):
        from .xsprep import _check_prep, frame_columns
        if combine is not None:
            from .combine import _check_spec
            _check_spec(combine)
        if turnover is not None:
            from .turnover import _check_spec as _check_turnover
            _check_turnover(turnover)
        self.turnover = turnover
        self.combine = combine
        self.prep = _check_prep(prep) if prep is not None else None
        self.groups = groups
        self.corr_method = check_corr_method(corr_method)
        self.layers = bool(layers)
        self.xcorr = bool(xcorr)
        self.factors_df = factors_df
        self.columns = frame_columns(factors_df, columns, groups)
        self.return_type = list(RETURN_TYPES)
        self.price_data = price_data
        self._res = None

    def run(self):
        import pandas as pd
        import torch
        fd = self.factors_df.reset_index()
        pdat = self.price_data.reset_index()
        dcol, icol = fd.columns[0], fd.columns[1]
        sd = fd[dcol].to_numpy().astype("datetime64[ns]")
        si = fd[icol].to_numpy().astype(np.int64)
        pd_ = pdat[pdat.columns[0]].to_numpy().astype("datetime64[ns]")
        pi_ = pdat[pdat.columns[1]].to_numpy().astype(np.int64)
        pc = pdat["close_price"].to_numpy(np.float64)
        dates = np.unique(np.concatenate([sd, pd_]))
        ids = np.unique(np.concatenate([si, pi_]))
        T, A, K = len(dates), len(ids), len(self.columns)
        lda = (A + 63) // 64 * 64
        dev = _dev()
        st = torch.from_numpy(np.searchsorted(dates, sd)).to(dev)
        sa = torch.from_numpy(np.searchsorted(ids, si)).to(dev)
        base = torch.full((K, T, lda), float("nan"), dtype=torch.float64, device=dev)
        vals = np.ascontiguousarray(fd[self.columns].to_numpy(np.float64).T)
        base[:, st, sa] = torch.from_numpy(vals).to(dev)
        rm = torch.zeros((T, lda), dtype=torch.bool, device=dev)
        rm[st, sa] = True
        pt = torch.from_numpy(np.searchsorted(dates, pd_)).to(dev)
        pa = torch.from_numpy(np.searchsorted(ids, pi_)).to(dev)
        close = torch.full((T, lda), float("nan"), dtype=torch.float64, device=dev)
        close[pt, pa] = torch.from_numpy(np.ascontiguousarray(pc)).to(dev)
        pm = torch.zeros((T, lda), dtype=torch.bool, device=dev)
        pm[pt, pa] = True
        year = dates.astype("datetime64[Y]").astype(np.int64) + 1970
        gplane, G = None, 0
        if self.prep is not None and self.prep.neutralize:
            from .xsprep import factorize_groups, frame_groups
            labels = frame_groups(self.factors_df, self.groups)
            if labels is None:
                raise ValueError("prep.neutralize needs groups")
            codes, G = factorize_groups(labels)
            gplane = torch.full((T, lda), -1, dtype=torch.int32, device=dev)
            gplane[st, sa] = torch.from_numpy(codes).to(dev)
        r = screen_grid(base, np.arange(K), close, pack_bits(pm), pack_bits(rm), A=A, year=year,
                        corr_method=self.corr_method, layers=self.layers, xcorr=self.xcorr,
                        prep=self.prep, groups=gplane, ngroups=max(G, 1), combine=self.combine,
                        turnover=self.turnover)
        r["dates"], r["ids"] = dates, ids
        self._res = r
        ic = r["ic"].cpu().numpy()                                   # [nd][K][3]
        nd = ic.shape[0]
        dts = pd.DatetimeIndex(dates[r["dates_idx"]])
        names = np.asarray(self.columns, dtype=object)
        types = np.asarray(self.return_type, dtype=object)
        keep = ~np.isnan(ic.reshape(-1))
        self.ic_df = pd.DataFrame({
            "date": np.repeat(dts.values, K * 3)[keep],
            "factor": np.tile(np.repeat(names, 3), nd)[keep],
            "Type": np.tile(types, nd * K)[keep],
            "IC": ic.reshape(-1)[keep]})
        ir = r["ir_year"].cpu().numpy()                              # [ny][K][3]
        ny = ir.shape[0]
        # a (year, factor, Type) row exists where the year has an IC (the reference's groupby)
        has = np.zeros((max(ny, 1), K, 3), dtype=bool)
        if nd:
            np.logical_or.at(has, r["years"] - r["year0"], ~np.isnan(ic))
        has = has[:ny].reshape(-1)
        self.ir_df = pd.DataFrame({
            "year": np.repeat(np.arange(ny, dtype=np.int64) + r["year0"], K * 3)[has],
            "factor": np.tile(np.repeat(names, 3), ny)[has],
            "Type": np.tile(types, ny * K)[has],
            "IR": ir.reshape(-1)[has]})
        st_ = r["stats"].cpu().numpy().reshape(K * 3, 5)
        key = np.abs(st_[:, 3])
        order = np.argsort(np.where(np.isnan(key), -np.inf, key) * -1.0, kind="stable")
        summary = pd.DataFrame(st_, columns=STATS)
        summary["n"] = summary["n"].astype(np.int64)
        summary.insert(0, "Type", np.tile(types, K))
        summary.insert(0, "factor", np.repeat(names, 3))
        self.summary = summary.iloc[order].reset_index(drop=True)
        if self.layers:
            self._layer_frames(dts, names, types)
        if self.xcorr:
            self._xcorr_frames()
        if self.prep is not None:
            from .xsprep import INFO
            info = r["prep_info"].cpu().numpy().reshape(nd * K, len(INFO))
            pi = pd.DataFrame(info, columns=INFO)
            for c in ("n", "n_lo", "n_hi"):
                pi[c] = pi[c].astype(np.int64)
            pi.insert(0, "factor", np.tile(names, nd))
            pi.insert(0, "date", np.repeat(dts.values, K))
            self.prep_info_df = pi
        if self.combine is not None:
            w = r["weights"].cpu().numpy()                           # [nd][K]
            keep = np.repeat(~np.isnan(w).all(axis=1), K)
            self.weights_df = pd.DataFrame({
                "date": np.repeat(dts.values, K)[keep],
                "factor": np.tile(names, nd)[keep],
                "weight": w.reshape(-1)[keep]})
            comp = pd.Series(r["composite"][st, sa].cpu().numpy(), index=self.factors_df.index,
                             name="composite")
            self.composite = comp.dropna()
            cs = pd.DataFrame(r["composite_stats"].cpu().numpy(), columns=STATS)
            cs["n"] = cs["n"].astype(np.int64)
            cs.insert(0, "Type", types)
            self.composite_summary = cs
        if self.turnover is not None:
            self._turnover_frames(dts, names)
        return self

    def _turnover_frames(self, dts, names):
        from .turnover import sort_summary, turnover_frames
        r, spec = self._res, self.turnover
        K, L = len(names), len(spec.lags)
        self.turnover_df, summary = turnover_frames(r, dts.values, names, spec)
        if self.layers and spec.lags[0] == 1:
            # the mean gross top-10 return_1 over the mean lag-1 turnover of the same book
            port = r["port"].cpu().numpy()[:, :, 0]                  # [nd][K]
            turn = r["turnover_stats"].cpu().numpy()[:, 0, 3, 1]     # [K]
            be = np.full((K, L), np.nan)
            for k in range(K):
                v = port[:, k][~np.isnan(port[:, k])]
                if len(v):
                    with np.errstate(all="ignore"):
                        be[k, 0] = np.float64(v.mean()) / turn[k]
            summary["breakeven_cost"] = be.reshape(-1)
        self.turnover_summary = sort_summary(summary, K, L)
        if self.combine is not None:
            _, cs = turnover_frames(r, dts.values, ["composite"], spec, prefix="composite_")
            self.composite_turnover_summary = cs.drop(columns="factor")

    def _xcorr_frames(self):
        import pandas as pd
        xs = self._res["xcorr_stats"].cpu().numpy()                 # [K][K][3]
        K, cols = len(self.columns), self.columns
        self.factor_corr = pd.DataFrame(xs[:, :, 1], index=cols, columns=cols)
        self.factor_corr_abs = pd.DataFrame(xs[:, :, 2], index=cols, columns=cols)
        self.factor_corr_n = pd.DataFrame(xs[:, :, 0].astype(np.int64), index=cols, columns=cols)
        ja, jb = np.triu_indices(K, 1)
        have = xs[ja, jb, 0] > 0
        ja, jb = ja[have], jb[have]
        order = np.argsort(-xs[ja, jb, 2], kind="stable")
        ja, jb = ja[order], jb[order]
        names = np.asarray(cols, dtype=object)
        self.redundant_pairs = pd.DataFrame({
            "factor_a": names[ja], "factor_b": names[jb], "mean": xs[ja, jb, 1],
            "mean_abs": xs[ja, jb, 2], "n": xs[ja, jb, 0].astype(np.int64)})

    def select(self, max_corr=0.7, k=None, return_type="return_1") -> list:
        """``select_factors`` on this screen: the columns by the \|whole-sample IR\| of
        ``return_type``, pruned by ``factor_corr_abs``."""
        if not self.xcorr or self._res is None:
            raise ValueError("select(): needs FactorScreen(..., xcorr=True).run()")
        q = self.return_type.index(return_type)
        ir = self._res["stats"].cpu().numpy()[:, q, 3]
        return select_factors(self.columns, ir, self.factor_corr_abs.to_numpy(), max_corr, k)

    def _layer_frames(self, dts, names, types):
        """The analyzer's _calc_layered_ret / _backtest_top_stocks frames (afm/analyzer.py) for
        every column at once."""
        import pandas as pd
        r = self._res
        nd, K = len(dts), len(names)
        cum = r["cum_layer"].cpu().numpy()                           # [nd][K][3][10]
        ls = r["ls"].cpu().numpy()                                   # [nd][K][3][5]
        port, cum_port = r["port"].cpu().numpy(), r["cum_port"].cpu().numpy()
        present = (r["layer_cnt"].cpu().numpy() > 0).any(axis=0)     # [K][10]: the factor's layers
        self.layered_ret_dfs, self.ls_ret_dfs = {}, {}
        for q, rt in enumerate(types):
            v = cum[:, :, q, :]
            keep = (present[None] & ~np.isnan(v)).reshape(-1)
            self.layered_ret_dfs[rt] = pd.DataFrame({
                "date": np.repeat(dts.values, K * 10)[keep],
                "factor": np.tile(np.repeat(names, 10), nd)[keep],
                "layer": np.tile(np.arange(1, 11, dtype=np.int64), nd * K)[keep],
                rt: v.reshape(-1)[keep]})
            v = ls[:, :, q, :]
            keep = ~np.isnan(v.reshape(-1))
            self.ls_ret_dfs[rt] = pd.DataFrame({
                "date": np.repeat(dts.values, K * 5)[keep],
                "factor": np.tile(np.repeat(names, 5), nd)[keep],
                "layer": np.tile(np.arange(5, 0, -1, dtype=np.int64), nd * K)[keep],
                rt: v.reshape(-1)[keep]})
        tnames = np.asarray(list(types) + [f"cum_{x}" for x in types], dtype=object)
        self.port_ret_df = pd.DataFrame({
            "date": np.repeat(dts.values, K * 6),
            "factor": np.tile(np.repeat(names, 6), nd),
            "Type": np.tile(tnames, nd * K),
            "Returns": np.concatenate([port, cum_port], axis=2).reshape(-1)})
        tmb = _last_valid(ls[:, :, :, 0]).reshape(-1)                # cum[10] - cum[1]
        mono = _layer_spearman(_last_valid(cum).reshape(K * 3, 10))
        topk = _last_valid(cum_port).reshape(-1)
        key = np.abs(tmb)
        order = np.argsort(np.where(np.isnan(key), -np.inf, key) * -1.0, kind="stable")
        ly = pd.DataFrame({"factor": np.repeat(names, 3), "Type": np.tile(types, K),
                           "top_minus_bottom": tmb, "monotonic": mono, "top_k": topk})
        self.layer_summary = ly.iloc[order].reset_index(drop=True)
