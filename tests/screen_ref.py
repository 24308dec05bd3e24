"""References of the factor-screening kernels (csrc/screen.hip): the reference's own pandas
statement of the per-date IC (KKT:342-349) and of the per-year IR (KKT:351-354) for every column,
a plain-Python restatement of pandas' nancorr recurrence, and the input builders the CPU and the
GPU tests share.  tests/test_screen_ref.py pins the restatement and the wide form to the per-column
pandas statement on the CPU.  Nothing here touches the GPU."""
import math
import os
import re
import warnings

import numpy as np
import pandas as pd

import analyzer_ref as R

RETURNS = list(R.RETURNS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constant(name: str) -> int:
    """An integer ``constexpr int <name> = <value>;`` of csrc/screen.hip."""
    src = open(os.path.join(ROOT, "alpha-multi-factor-models_amd", "csrc", "screen.hip")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


# ---- the per-date IC ------------------------------------------------------------------------------
def ic_pandas(f: np.ndarray, rets: np.ndarray) -> np.ndarray:
    """One date, one column (KKT:344-345): f [n], rets [3][n] -> DataFrame.corr(method='pearson')
    of [factor, return_1, return_2, return_5], the factor's row without itself: [3]."""
    df = pd.DataFrame(dict(zip(R.COLS, [f, *rets])))
    with np.errstate(all="ignore"):
        return df.corr(method="pearson")["f"].to_numpy()[1:]


def ic_pandas_wide(F: np.ndarray, rets: np.ndarray) -> np.ndarray:
    """One date, every column at once: F [K][n] -> [K][3].  One corr() of the frame [f_0 ..
    f_K-1, return_1, return_2, return_5]: nancorr treats every pair on its own rows and in the
    same orientation (the return is the later column), so the (f_k, return_q) entries are those of
    ``ic_pandas`` (pinned in tests/test_screen_ref.py)."""
    K = F.shape[0]
    df = pd.DataFrame(np.concatenate([F, rets]).T)
    with np.errstate(all="ignore"):
        return df.corr(method="pearson").to_numpy()[:K, K:]


def ic_recurrence(f: np.ndarray, rets: np.ndarray) -> np.ndarray:
    """pandas' nancorr for (x = return q, y = factor) restated in plain Python floats: rows in
    order, a row skipped when either value is not finite, Welford means and sums of squared
    deviations, covxy / sqrt(ssqdm_x * ssqdm_y), NaN when the divisor is 0 or no row is left."""
    out = np.full(3, np.nan)
    for q in range(3):
        nobs = 0
        mx = my = sxx = syy = sxy = 0.0
        for vx, vy in zip(rets[q].tolist(), np.asarray(f, dtype=np.float64).tolist()):
            if math.isfinite(vx) and math.isfinite(vy):
                nobs += 1
                dx, dy = vx - mx, vy - my
                mx += 1.0 / nobs * dx
                my += 1.0 / nobs * dy
                sxx += (vx - mx) * dx
                syy += (vy - my) * dy
                sxy += (vx - mx) * dy
        if nobs >= 1:
            div = math.sqrt(sxx * syy)
            if div != 0:
                out[q] = sxy / div
    return out


# ---- the summary ----------------------------------------------------------------------------------
def summary_pandas(ic: np.ndarray, year: np.ndarray, nyears: int, year0: int):
    """ic [nd][K][3] -> stats [K][3][5] = (n, mean, std, mean / std, that * sqrt(n)) of each
    column's non-NaN ICs in pandas, ir_year [nyears][K][3] = ``series_pandas``' IR per column."""
    nd, K, _ = ic.shape
    stats = np.full((K, 3, 5), np.nan)
    ir_year = np.full((nyears, K, 3), np.nan)
    zl, zp = np.zeros((nd, 3, 10)), np.zeros((nd, 3))
    for k in range(K):
        for q in range(3):
            s = pd.Series(ic[:, k, q]).dropna()
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                n, mean, std = len(s), s.mean(), s.std()
                ir = mean / std
                stats[k, q] = [n, mean, std, ir, ir * np.sqrt(np.float64(n))]
        if nd:
            ir_year[:, k, :] = R.series_pandas(zl, zp, ic[:, k, :], year, nyears, year0)[3]
    return stats, ir_year


# ---- inputs of the kernel tests ---------------------------------------------------------------------
LDA = 1600
# rows per date: STAT_COUNTS' edges plus 0 and every asset
COUNTS_A = (0, 1, 2, 63, 64, 65, 511, 512, 513, 1025, 1537, LDA)


def counts_chunk_edges():
    """Both sides of the staging-chunk edge of screen_ic_kernel (kScreenRows rows per chunk: one
    chunk, two, three -- the prefetch of the asset indices runs two chunks ahead) and of its
    1 / row-number ring (kScreenInv rows), from the kernel's constants."""
    rows, inv = kernel_constant("kScreenRows"), kernel_constant("kScreenInv")
    c = []
    for e in (rows, 2 * rows, 3 * rows, inv, 2 * inv + rows):
        c += [e - 1, e, e + 1]
    return tuple(c)


def screen_inputs(counts, kind: str, P: int = 130, lda: int = LDA, seed: int = 61):
    """planes [P][T][lda], rows [4][T][lda], rows_idx [T][lda], nrows [T] with ``counts`` rows
    per date.  rows_idx: ascending, with gaps, the last asset in every date of two or more rows;
    every cell of the planes is finite unless the kind says so (the cells outside rows_idx, the
    padding columns among them, must not be read as rows); rows' plane 0 is NaN (unused), its
    cells past nrows finite.  Kinds: 'finite' (even planes rounded: ties; plane 5 constant on
    every date, plane 70 constant on the 512- and 64-row dates); 'inf' (+-inf / NaN in planes 3,
    64, 66 and 129 only: first chunk only, a later chunk only, the last row); 'retinf' ('inf'
    plus inf in return_2 alone on two dates and in return_1 on another)."""
    rng = np.random.default_rng(seed)
    T = len(counts)
    planes = rng.normal(size=(P, T, lda))
    planes[::2] = np.round(planes[::2], 2)
    rows = rng.normal(size=(4, T, lda)) * 0.02
    rows[0] = np.nan
    rows_idx = np.full((T, lda), -1, dtype=np.int32)
    for t, n in enumerate(counts):
        if n == lda:
            idx = np.arange(lda)
        elif n >= 2:
            idx = np.r_[np.sort(rng.permutation(lda - 1)[:n - 1]), lda - 1]
        else:
            idx = np.sort(rng.permutation(lda - 1)[:n])
        rows_idx[t, :n] = idx
    if kind == "finite":
        planes[5] = 0.75
        for t, n in enumerate(counts):
            if n in (512, 64):
                planes[70, t] = -2.0
    else:
        chunk = kernel_constant("kScreenRows")
        for t, n in enumerate(counts):
            idx = rows_idx[t, :n]
            if n >= 1:
                planes[3, t, idx[n - 1]] = np.inf                    # the last row
            if n >= 3:
                planes[64, t, idx[[0, min(2, chunk - 1)]]] = [-np.inf, np.nan]   # first chunk only
            if n > chunk:
                planes[66, t, idx[chunk:min(n, chunk + 3)]] = np.nan   # a later chunk only
                planes[129, t, idx[n - 1]] = -np.inf
                planes[129, t, idx[0]] = np.inf
        if kind == "retinf":
            for t, n in enumerate(counts):
                if n in (1537, 65, 2):
                    rows[2, t, [0, n - 1]] = [np.inf, -np.inf]       # return_2 alone
                if n == 513:
                    rows[1, t, 300] = np.inf
        else:
            assert kind == "inf"
    return planes, rows, rows_idx, np.array(counts, dtype=np.int32)


def zs_table(P: int, lda: int = LDA, seed: int = 67):
    """zs [P][lda][2] = {mu, 1/sd}; row 7 unusable ({0, 0}) on every asset."""
    rng = np.random.default_rng(seed)
    zs = np.stack([rng.normal(size=(P, lda)), np.exp(rng.normal(size=(P, lda)))], axis=-1)
    zs[7] = 0.0
    return np.ascontiguousarray(zs)


def screen_ref(planes, rows, rows_idx, nrows, zs=None):
    """ic [T][P][3] of every date and plane in pandas; with zs the values are (x - mu) * inv of
    the plane's own row of the table, in numpy."""
    P, T, _ = planes.shape
    ic = np.full((T, P, 3), np.nan)
    for t in range(T):
        n = int(nrows[t])
        if n == 0:
            continue
        idx = rows_idx[t, :n]
        F = planes[:, t, idx]
        if zs is not None:
            with np.errstate(all="ignore"):
                F = (F - zs[:, idx, 0]) * zs[:, idx, 1]
        ic[t] = ic_pandas_wide(F, rows[1:, t, :n])
    return ic
