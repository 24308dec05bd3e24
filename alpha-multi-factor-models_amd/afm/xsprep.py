"""Cross-sectional factor preprocessing: what a multi-factor workflow does to a factor across the
securities of one date before it is rated or regressed -- winsorise (median +- n MAD, or two
quantiles), take out the group (sector) mean, standardise to mean 0 and sd 1 -- for every column
and date in one launch (csrc/xsprep.hip, include/afm_xsprep.h).

In pandas, per column ``c`` with its missing cells dropped::

    g = df[c].dropna().groupby('date')
    x = clip to g.median() +- n * 1.4826 * MAD      (or to g.quantile(q_lo), g.quantile(q_hi))
    x = x - x.groupby(['date', sector]).transform('mean')
    x = (x - g.transform('mean')) / g.transform('std')

``XsPrep`` names the steps, ``preprocess_grid`` runs them on device grids (the factor screen's
stage in front of its IC / layers / correlation kernels: ``screen_grid(..., prep=...)``) and
``preprocess_factors`` is the frame interface.

Out of scope: the multi-GPU pipeline, regression-based neutralisation.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from .analyzer import _buffer, _dev

WINSOR_MODES = {None: 0, "mad": 1, "quantile": 2}
MAD_SCALE = 1.4826                 # MAD -> sd of a normal distribution
MAX_GROUPS = 256
INFO = ["n", "lo", "hi", "n_lo", "n_hi", "mean", "std"]


@dataclass(frozen=True)
class XsPrep:
    """The per-date preprocessing of a factor column, applied in this order: ``winsor`` (None,
    'mad': clip to median +- ``n_mad`` * 1.4826 * MAD, no clipping where the MAD is 0; 'quantile':
    clip to the ``quantiles`` (q_lo, q_hi) of numpy's linear method), ``neutralize`` (subtract the
    mean of the row's group on the date), ``standardize`` (mean 0, sd 1 with ddof = 1 across the
    date; NaN where the date has fewer than two rows or no spread)."""
    winsor: str | None = None
    n_mad: float = 3.0
    quantiles: tuple = (0.01, 0.99)
    neutralize: bool = False
    standardize: bool = True

    def __post_init__(self):
        if self.winsor not in WINSOR_MODES:
            raise ValueError(f"winsor={self.winsor!r}: expected None, 'mad' or 'quantile'")
        n_mad = float(self.n_mad)
        if not (math.isfinite(n_mad) and n_mad > 0):
            raise ValueError(f"n_mad={self.n_mad!r}: expected a finite positive number")
        try:
            q_lo, q_hi = (float(q) for q in self.quantiles)
        except (TypeError, ValueError):
            raise ValueError(f"quantiles={self.quantiles!r}: expected (q_lo, q_hi)") from None
        if not 0.0 <= q_lo < q_hi <= 1.0:
            raise ValueError(f"quantiles={self.quantiles!r}: expected 0 <= q_lo < q_hi <= 1")
        object.__setattr__(self, "n_mad", n_mad)
        object.__setattr__(self, "quantiles", (q_lo, q_hi))
        object.__setattr__(self, "neutralize", bool(self.neutralize))
        object.__setattr__(self, "standardize", bool(self.standardize))

    @property
    def mode(self) -> int:
        return WINSOR_MODES[self.winsor]

    @property
    def flags(self) -> int:
        return int(self.neutralize) | int(self.standardize) << 1

    @property
    def params(self) -> tuple:
        """(p_lo, p_hi) of afm_xs_preprocess_f64."""
        if self.winsor == "mad":
            c = self.n_mad * MAD_SCALE
            return c, c
        if self.winsor == "quantile":
            return self.quantiles
        return 0.0, 0.0


def _check_prep(prep) -> XsPrep:
    if not isinstance(prep, XsPrep):
        raise TypeError(f"prep: expected an XsPrep, got {type(prep).__name__}")
    return prep


def preprocess_grid(base, cols, rows_idx, nrows, dates_idx, *, T: int, lda: int, prep: XsPrep,
                    zs=None, zcols=None, col_stride=None, groups=None, ngroups: int = 0,
                    out=None, bufs=None) -> dict:
    """Device-level preprocessing on grids.  ``base``, ``cols``, ``zs``, ``zcols``,
    ``col_stride``: the planes and values of ``screen_grid``; ``rows_idx`` [T][lda] / ``nrows``
    [T] (int32): the compacted asset indices of each date's rows; ``dates_idx``: the evaluated
    dates.  ``groups``: int32 labels [lda] (one per asset) or [T][lda], in [0, ``ngroups``) --
    a row with another label is missing when ``prep.neutralize``.

    Returns device tensors ``out`` [K][T][lda] -- for an evaluated date the whole row: the result
    on the rows that are present for the column, NaN elsewhere; the rows of other dates are left
    as they are (NaN in a buffer allocated here) -- and ``info`` [nd][K][7] = (n, lo, hi, n_lo,
    n_hi, mean, std).  ``out`` / ``bufs``: a tensor to write into / a dict that keeps the buffers
    between calls (``prep_out``, ``prep_info``)."""
    import torch
    prep = _check_prep(prep)
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
    zc_t = dev_i32(zcols) if zcols is not None else None
    d_t = dev_i32(dates_idx)
    nd = int(d_t.numel())
    if col_stride is None:
        col_stride = T * lda
    g_stride = 0
    if prep.neutralize:
        if groups is None:
            raise ValueError("prep.neutralize needs groups")
        groups = dev_i32(groups)
        if tuple(groups.shape) == (T, lda):
            g_stride = lda
        elif tuple(groups.shape) != (lda,):
            raise ValueError(f"groups: expected shape ({lda},) or ({T}, {lda}), got "
                             f"{tuple(groups.shape)}")
    else:
        groups, ngroups = None, 0
    if out is None:
        kept = bufs.get("prep_out") if bufs is not None else None
        out = _buffer(bufs, "prep_out", (K, T, lda), f64, dev)
        if out is not kept:                                # allocated here
            out.fill_(float("nan"))
    info = _buffer(bufs, "prep_info", (nd, K, 7), f64, dev)
    p_lo, p_hi = prep.params
    ctx.call("afm_xs_preprocess_f64", base, col_stride, T, lda, cols_t, K, zs, zc_t, d_t, nd,
             rows_idx, nrows, groups, g_stride, ngroups, prep.mode, p_lo, p_hi, prep.flags, out,
             T * lda, info if nd else None)
    return {"out": out, "info": info}


def rows_of_mask(mask):
    """``mask`` [T][lda] bool (device) -> (rows_idx [T][lda] int32, nrows [T] int32): the asset
    indices of each date's rows, ascending, compacted to the front."""
    import torch
    T, lda = mask.shape
    nrows = mask.sum(dim=1)
    t, a = torch.nonzero(mask, as_tuple=True)              # (date, asset) in lexicographic order
    start = torch.cumsum(nrows, 0) - nrows
    rows_idx = torch.zeros((T, lda), dtype=torch.int32, device=mask.device)
    rows_idx[t, torch.arange(t.numel(), device=mask.device) - start[t]] = a.to(torch.int32)
    return rows_idx, nrows.to(torch.int32)


def factorize_groups(labels) -> tuple:
    """Labels of any dtype -> (int32 codes in 0..G-1 in order of first appearance, NaN / None ->
    -1; G)."""
    import pandas as pd
    codes, uniques = pd.factorize(np.asarray(labels), sort=False)
    if len(uniques) > MAX_GROUPS:
        raise ValueError(f"groups: {len(uniques)} distinct labels (at most {MAX_GROUPS})")
    return codes.astype(np.int32), len(uniques)


def frame_groups(factors_df, groups):
    """``groups`` of the frame interfaces -- a Series on the frame's (date, id) index or the name
    of one of its columns -> the labels of the frame's rows (an array), or None."""
    import pandas as pd
    if groups is None:
        return None
    if isinstance(groups, pd.Series):
        if len(groups) != len(factors_df) or not groups.index.equals(factors_df.index):
            groups = groups.reindex(factors_df.index)
        return groups.to_numpy()
    if isinstance(groups, str) or not hasattr(groups, "__len__"):
        if groups not in factors_df.columns:
            raise ValueError(f"groups={groups!r} is not a column of the frame")
        return factors_df[groups].to_numpy()
    if len(groups) != len(factors_df):
        raise ValueError("groups: one label per row of the frame")
    return np.asarray(groups)


def frame_columns(factors_df, columns, groups) -> list:
    """The factor columns of a frame interface: ``columns``, or every column but the one
    ``groups`` names."""
    if columns is not None:
        return list(columns)
    skip = groups if isinstance(groups, str) else None
    return [c for c in factors_df.columns if skip is None or c != skip]


def preprocess_factors(factors_df, columns=None, groups=None, prep=XsPrep()):
    """``preprocess_factors(factors_df, columns=None, groups=None, prep=XsPrep())``: the per-date
    preprocessing of the columns of ``factors_df`` -- indexed (date, id), one column per factor --
    on the GPU: the drop-in for ``df.groupby('date').transform(...)`` per column before an OLS /
    Fama-MacBeth fit or a ``FactorScreen``.  The row set of a date is the frame's rows of that
    date; a NaN or inf cell is missing for its own column only.  ``groups``: the sector of every
    row, a Series on the same index or the name of a column of the frame (then not a factor), of
    any dtype; a NaN label puts the row outside every group (missing when ``prep.neutralize``).

    Returns a copy of the frame, index and column order kept, with the chosen columns replaced by
    their preprocessed values (float64; NaN where the cell is missing for its column)."""
    import torch
    prep = _check_prep(prep)
    cols = frame_columns(factors_df, columns, groups)
    labels = frame_groups(factors_df, groups)
    if prep.neutralize and labels is None:
        raise ValueError("prep.neutralize needs groups")
    out_df = factors_df.copy()
    if not len(cols) or not len(factors_df):
        return out_df
    dcol = factors_df.index.get_level_values(0).to_numpy()
    icol = factors_df.index.get_level_values(1).to_numpy()
    dates, t_idx = np.unique(dcol, return_inverse=True)
    ids, a_idx = np.unique(icol, return_inverse=True)
    T, A, K = len(dates), len(ids), len(cols)
    lda = (A + 63) // 64 * 64
    if lda > 32768:
        raise ValueError(f"{A} securities: at most 32768")
    dev = _dev()
    st = torch.from_numpy(t_idx.astype(np.int64)).to(dev)
    sa = torch.from_numpy(a_idx.astype(np.int64)).to(dev)
    base = torch.full((K, T, lda), float("nan"), dtype=torch.float64, device=dev)
    vals = np.ascontiguousarray(factors_df[cols].to_numpy(np.float64).T)
    base[:, st, sa] = torch.from_numpy(vals).to(dev)
    mask = torch.zeros((T, lda), dtype=torch.bool, device=dev)
    mask[st, sa] = True
    rows_idx, nrows = rows_of_mask(mask)
    gplane, G = None, 0
    if prep.neutralize:
        codes, G = factorize_groups(labels)
        gplane = torch.full((T, lda), -1, dtype=torch.int32, device=dev)
        gplane[st, sa] = torch.from_numpy(codes).to(dev)
    r = preprocess_grid(base, np.arange(K), rows_idx, nrows, np.arange(T), T=T, lda=lda,
                        prep=prep, groups=gplane, ngroups=max(G, 1))
    got = r["out"][:, st, sa].cpu().numpy()                # [K][rows of the frame]
    for k, c in enumerate(cols):
        out_df[c] = got[k]
    return out_df
