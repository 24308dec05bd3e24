"""Restatements of the cross-sectional preprocessing (include/afm_xsprep.h) and the inputs the
tests share -- a plain module, pinned on the CPU by tests/test_xsprep_ref.py.

``item_f64``: the steps in numpy float64 -- the median via np.median, the quantiles via
np.quantile, the group means and the moments via pandas (groupby.transform('mean'), Series.mean /
.std), the missing cells of the column dropped first.  ``item_ld``: steps 2 and 3 again in
np.longdouble on the same winsorised values (the order statistics of step 1 are exact values and
are taken from float64), rounded to double at the end.  ``E64`` of an item is the largest distance
between the two; the engine has to stay within ``tolerance`` of the long-double one."""
import functools

import numpy as np
import pandas as pd

LD = np.longdouble
NEUTRALIZE, STANDARDIZE = 1, 2
MAD_C = 3.0 * 1.4826
EPS = 2.0 ** -53

# the column families of the kernel tests, one plane each
FAMILIES = ["normal", "offset", "small", "ties", "const", "two", "holes", "allmiss", "zeros", "psy"]
NORMAL, OFFSET, SMALL, TIES, CONST, TWO, HOLES, ALLMISS, ZEROS, PSY = range(10)
SMALL_COUNTS = [0, 1, 2, 3, 4, 63, 64, 65, 511, 512, 513]


def quantile_lerp(s, q):
    """numpy's linear quantile of the sorted float64 array ``s``, written out."""
    n = len(s)
    v = np.float64(n - 1) * np.float64(q)
    i = int(np.floor(v))
    g = v - np.floor(v)
    a, b = s[i], s[min(i + 1, n - 1)]
    with np.errstate(all="ignore"):
        return a + (b - a) * g if g < 0.5 else b - (b - a) * (1.0 - g)


def step1(x, winsor, p_lo, p_hi):
    """x: the finite values of the item -> (lo, hi, w, n_lo, n_hi)."""
    n = len(x)
    with np.errstate(all="ignore"):
        if winsor == 0:
            lo, hi = -np.inf, np.inf
        elif n == 0:
            lo = hi = np.nan
        elif winsor == 1:
            med = np.median(x)
            mad = np.median(np.abs(x - med))
            lo, hi = (med - p_lo * mad, med + p_hi * mad) if mad != 0 else (-np.inf, np.inf)
        else:
            lo, hi = np.quantile(x, p_lo), np.quantile(x, p_hi)
        w = np.minimum(np.maximum(x, lo), hi) if n else x
        return float(lo), float(hi), w, int((x < lo).sum()), int((x > hi).sum())


def steps23_f64(w, g, flags):
    """-> (out, mu, sd) in float64 with pandas."""
    v = pd.Series(w, dtype=np.float64)
    n = len(v)
    if flags & NEUTRALIZE and n:
        v = v - v.groupby(np.asarray(g)).transform("mean")
    mu = sd = np.nan
    if flags & STANDARDIZE:
        with np.errstate(all="ignore"):
            mu = float(v.mean()) if n else np.nan
            sd = float(v.std()) if n >= 2 else np.nan
            if n < 2 or not np.isfinite(sd) or sd == 0:
                v = pd.Series(np.full(n, np.nan))
            else:
                v = (v - mu) / sd
    return v.to_numpy(np.float64), mu, sd


def steps23_ld(w, g, flags):
    """-> (out, mu, sd) in long double (numpy's pairwise sums), rounded to double."""
    v = np.asarray(w, dtype=LD)
    n = len(v)
    if flags & NEUTRALIZE and n:
        g = np.asarray(g)
        order = np.argsort(g, kind="stable")
        bounds = np.flatnonzero(np.r_[True, g[order][1:] != g[order][:-1], True])
        out = np.empty(n, dtype=LD)
        for s, e in zip(bounds[:-1], bounds[1:]):
            idx = order[s:e]
            out[idx] = v[idx] - np.sum(v[idx]) / LD(e - s)
        v = out
    mu = sd = LD(np.nan)
    if flags & STANDARDIZE:
        with np.errstate(all="ignore"):
            if n:
                mu = np.sum(v) / LD(n)
            if n >= 2:
                sd = np.sqrt(np.sum((v - mu) ** 2) / LD(n - 1))
            if n < 2 or not np.isfinite(sd) or sd == 0:
                v = np.full(n, np.nan, dtype=LD)
            else:
                v = (v - mu) / sd
    return v.astype(np.float64), float(mu), float(sd)


def item(x, g, ngroups, winsor, p_lo, p_hi, flags):
    """One (date, column): ``x`` the values at the date's rows (float64, missing cells included),
    ``g`` their group labels (or None).  -> dict: out64 / outld [len(x)] (NaN where missing),
    info64 / infold [7], E64."""
    x = np.asarray(x, dtype=np.float64)
    ok = np.isfinite(x)
    if flags & NEUTRALIZE:
        g = np.asarray(g)
        ok &= (g >= 0) & (g < ngroups)
    xf = x[ok]
    gf = g[ok] if flags & NEUTRALIZE else None
    lo, hi, w, n_lo, n_hi = step1(xf, winsor, p_lo, p_hi)
    res = {}
    for name, fn in (("64", steps23_f64), ("ld", steps23_ld)):
        o, mu, sd = fn(w, gf, flags)
        out = np.full(len(x), np.nan)
        out[ok] = o
        res["out" + name] = out
        res["info" + name] = np.array([len(xf), lo, hi, n_lo, n_hi, mu, sd], dtype=np.float64)
    both = ~np.isnan(res["out64"]) & ~np.isnan(res["outld"])
    res["E64"] = float(np.abs(res["out64"][both] - res["outld"][both]).max()) if both.any() else 0.0
    return res


def tolerance(E64, ref):
    """The bound of the issue: max(4 E64, 16 * 2^-53 * max(1, max |ref|)) of one item."""
    m = float(np.nanmax(np.abs(ref))) if np.isfinite(ref).any() else 0.0
    return max(4.0 * E64, 16.0 * EPS * max(1.0, m))


def values(planes, cols, t, idx, zs=None, zcols=None):
    """x [K][n]: what the engine reads for the rows ``idx`` of date ``t`` (z on the fly: the
    expression (x - mu) * (1/sd) of csrc/screen.hip)."""
    out = []
    for k, c in enumerate(cols):
        x = planes[c, t, idx]
        if zs is not None:
            zr = zs[zcols[k] if zcols is not None else k]
            with np.errstate(all="ignore"):
                x = (x - zr[idx, 0]) * zr[idx, 1]
        out.append(x)
    return out


def call_ref(planes, cols, rows_idx, nrows, dates, groups, ngroups, winsor, p_lo, p_hi, flags,
             zs=None, zcols=None):
    """The whole call -> out64 / outld [K][nd][lda] (row i: evaluated date i, NaN off the rows),
    info64 / infold [nd][K][7], E64 [nd][K]."""
    K, nd, lda = len(cols), len(dates), planes.shape[2]
    r = {k: np.full((K, nd, lda), np.nan) for k in ("out64", "outld")}
    r.update({k: np.zeros((nd, K, 7)) for k in ("info64", "infold")})
    r["E64"] = np.zeros((nd, K))
    for i, t in enumerate(dates):
        idx = rows_idx[t, :nrows[t]]
        g = None
        if flags & NEUTRALIZE:
            g = (groups[t] if groups.ndim == 2 else groups)[idx]
        for k, x in enumerate(values(planes, cols, t, idx, zs, zcols)):
            it = item(x, g, ngroups, winsor, p_lo, p_hi, flags)
            for name in ("out64", "outld"):
                r[name][k, i, idx] = it[name]
            r["info64"][i, k], r["infold"][i, k], r["E64"][i, k] = it["info64"], it["infold"], it["E64"]
    return r


# ---- inputs -------------------------------------------------------------------------------------
def family_planes(rng, T, lda):
    """[10][T][lda]: one plane per family of FAMILIES, defined on every cell."""
    P = np.empty((len(FAMILIES), T, lda))
    z = rng.normal(size=(T, lda))
    P[NORMAL] = z
    P[OFFSET] = 1e6 + rng.normal(size=(T, lda))
    P[SMALL] = 1e-4 * rng.normal(size=(T, lda))
    levels = np.round(np.linspace(-2.1, 2.1, 15), 1)               # heavy ties: a set of 15
    P[TIES] = levels[rng.integers(0, 15, size=(T, lda))]
    P[CONST] = 1.5
    P[TWO] = np.where(rng.random((T, lda)) < 0.4, -0.75, 2.5)
    h = rng.normal(size=(T, lda))
    u = rng.random((T, lda))
    h[u < 0.05] = np.nan
    h[(u >= 0.05) & (u < 0.06)] = np.inf
    h[(u >= 0.06) & (u < 0.07)] = -np.inf
    P[HOLES] = h
    P[ALLMISS] = np.nan
    zc = rng.integers(0, 8, size=(T, lda))
    P[ZEROS] = np.select([zc < 3, zc < 6, zc == 6], [0.0, -0.0, 1.0], -1.0)
    P[PSY] = np.where(rng.random((T, lda)) < 0.6, 50.0, 50.0 + 10 * rng.normal(size=(T, lda)))
    return P


def row_sets(rng, counts, lda):
    """rows_idx [T][lda] / nrows [T] for the row counts: ascending assets with gaps, the last asset
    among them; one date (the largest below lda) in shuffled order."""
    T = len(counts)
    rows_idx = np.zeros((T, lda), dtype=np.int32)
    shuffled = max((n for n in counts if n < lda), default=-1)
    for t, n in enumerate(counts):
        if n >= lda:
            idx = np.arange(lda)
        else:
            idx = np.sort(rng.choice(lda - 1, size=n, replace=False))
            if n:
                idx[-1] = lda - 1
        if n == shuffled and n > 2:
            idx = rng.permutation(idx)
        rows_idx[t, :n] = idx
    return rows_idx, np.asarray(counts, dtype=np.int32)


def group_labels(rng, shape, G, bad=True):
    """int32 labels in [0, G): with ``bad`` 3 % are -1, 3 % G and 1 % G + 5 (outside); for G > 1
    the last label belongs to the last asset alone (a group of one row: row_sets puts that asset
    on every date)."""
    g = rng.integers(0, max(G - 1, 1), size=shape).astype(np.int32)
    if bad:
        u = rng.random(shape)
        g[u < 0.03] = -1
        g[(u >= 0.03) & (u < 0.06)] = G
        g[(u >= 0.06) & (u < 0.07)] = G + 5
    if G > 1:
        g[..., -1] = G - 1
    return g


@functools.lru_cache(maxsize=None)
def small_case():
    """The row counts 0 .. 513 plus a date that is never evaluated, lda = 576."""
    rng = np.random.default_rng(2024)
    counts = SMALL_COUNTS + [40]
    lda = 576
    planes = family_planes(rng, len(counts), lda)
    rows_idx, nrows = row_sets(rng, counts, lda)
    for a in (planes, rows_idx, nrows):
        a.setflags(write=False)
    return planes, rows_idx, nrows


@functools.lru_cache(maxsize=None)
def large_case(n_hi: int):
    """Two dates of n_hi - 1 and n_hi rows (the border of an instantiation: n_hi = 4097, 12289)
    or one date of 32768 rows, lda the next multiple of 64."""
    rng = np.random.default_rng(n_hi)
    counts = [n_hi] if n_hi == 32768 else [n_hi - 1, n_hi]
    lda = (n_hi + 63) // 64 * 64
    planes = family_planes(rng, len(counts), lda)
    rows_idx, nrows = row_sets(rng, counts, lda)
    for a in (planes, rows_idx, nrows):
        a.setflags(write=False)
    return planes, rows_idx, nrows


def zs_table(rng, P, lda):
    """[P][lda][2] = {mu, 1/sd} per (plane, asset), as afm_zstats_finalize_f64 leaves it."""
    zs = np.empty((P, lda, 2))
    zs[:, :, 0] = rng.normal(size=(P, lda))
    zs[:, :, 1] = 1.0 / rng.uniform(0.5, 2.0, size=(P, lda))
    return zs
