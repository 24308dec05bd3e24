"""The factor risk model of include/afm_risk.h stated in numpy: the arithmetic the kernels of
csrc/risk.hip equal bit for bit.  Every operator is one IEEE fp64 operation and every sum adds its
terms in the header's order (the loops below ARE that order; vectorised only across independent
elements).  Also the closed forms in longdouble that tests/test_risk_ref.py holds the recurrences
against."""
import numpy as np


LD = np.longdouble


def decay(half_life, dtype=np.float64):
    if dtype is np.float64:
        return 0.5 ** (1.0 / float(half_life))
    return dtype(0.5) ** (dtype(1.0) / dtype(half_life))


def used_dates(beta, rank):
    """[T] bool: no regressor dropped and every coefficient finite."""
    beta = np.asarray(beta, dtype=np.float64)
    return (np.asarray(rank) == beta.shape[1] - 1) & np.isfinite(beta).all(axis=1)


def residuals(X, y, mask, beta, rank):
    """X [p][T][A], y [T][A], mask [T][A] bool (the row bits), beta [T][p+1], rank [T] -> u [T][A]."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    used = used_dates(beta, rank)
    with np.errstate(all="ignore"):
        acc = np.repeat(beta[:, :1], y.shape[1], axis=1)
        for j in range(X.shape[0]):
            acc = acc + beta[:, j + 1:j + 2] * X[j]
        u = y - acc
    ok = mask & used[:, None] & np.isfinite(y) & np.isfinite(X).all(axis=0)
    return np.where(ok, u, np.nan)


def factor_cov(beta, rank, half_life, min_obs, lag, dtype=np.float64):
    """-> (fcov [T][K1][K1], nused [T] int32): West's weighted update over the used dates.
    ``dtype``: the same recurrence in another precision (tests/test_risk_ref.py: longdouble)."""
    used = used_dates(beta, rank)
    beta = np.asarray(beta, dtype=dtype)
    T, K1 = beta.shape
    lam = decay(half_life, dtype)
    fcov = np.full((T, K1, K1), np.nan, dtype=dtype)
    nused = np.zeros(T, dtype=np.int32)
    W, m, C, cnt = dtype(0.0), np.zeros(K1, dtype=dtype), np.zeros((K1, K1), dtype=dtype), 0
    for s in range(T):
        if used[s]:
            lw = lam * W
            Wn = lw + dtype(1.0)
            g = lw / Wn
            d = beta[s] - m
            m = m + d / Wn
            full = lam * C + (g * d)[:, None] * d[None, :]
            C = np.tril(full) + np.tril(full, -1).T             # i >= j, mirrored
            W = Wn
            cnt += 1
        if s + lag < T:
            nused[s + lag] = cnt
            if cnt >= min_obs:
                fcov[s + lag] = C / W
    return fcov, nused


def np_sum(v):
    """np.add.reduce of a contiguous vector: numpy itself."""
    return float(np.add.reduce(np.ascontiguousarray(v, dtype=np.float64)))


def _pairwise(a):
    n = len(a)
    if n < 8:
        res = 0.0
        for x in a:
            res = res + float(x)
        return res
    if n <= 128:
        r = [float(x) for x in a[:8]]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = r[j] + float(a[i + j])
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for x in a[i:]:
            res = res + float(x)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a[:n2]) + _pairwise(a[n2:])


def np_sum_stated(v):
    """The order include/afm_risk.h gives for np_sum, spelled out: +0.0, then numpy's pairwise sum of
    each run of 8192 values added in order (tests/test_risk_ref.py holds it against numpy)."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    r = 0.0
    for c0 in range(0, len(v), 8192):
        r = r + _pairwise(v[c0:c0 + 8192])
    return r


def specific(u, half_life, min_obs, lag, dtype=np.float64):
    """u [T][A] -> (spec [T][A], fill [T]).  ``dtype``: as in factor_cov (fill stays fp64's)."""
    u = np.asarray(u, dtype=dtype)
    T, A = u.shape
    lam = decay(half_life, dtype)
    spec = np.full((T, A), np.nan, dtype=dtype)
    W, D, n = np.zeros(A, dtype=dtype), np.zeros(A, dtype=dtype), np.zeros(A, dtype=np.int64)
    for s in range(T):
        f = np.isfinite(u[s])
        us = np.where(f, u[s], dtype(0.0))
        W = np.where(f, lam * W + dtype(1.0), W)
        D = np.where(f, lam * D + us * us, D)
        n = n + f
        if s + lag < T:
            with np.errstate(all="ignore"):
                spec[s + lag] = np.where(n >= min_obs, D / W, np.nan)
    fill = np.full(T, np.nan)
    for t in range(T):
        v = spec[t][np.isfinite(spec[t])]
        if len(v):
            fill[t] = np_sum(v) / float(len(v))
    return spec, fill


def exposures(X, t, members):
    """B [k][K1]: the intercept, then x_j at (t, a_m); a non-finite exposure counts as 0."""
    members = np.asarray(members, dtype=np.int64)
    B = np.ones((len(members), X.shape[0] + 1))
    if len(members):
        v = X[:, t, members].T
        B[:, 1:] = np.where(np.isfinite(v), v, 0.0)
    return B


def net_book(long_ids, wl, short_ids, ws):
    """The union (long members, then the short members not among them) and h = (w_L - w_S) / 2."""
    long_ids, short_ids = [int(a) for a in long_ids], [int(a) for a in short_ids]
    mem, h = [], []
    for m, a in enumerate(long_ids):
        s = ws[short_ids.index(a)] if a in short_ids else 0.0
        mem.append(a)
        h.append((wl[m] - s) / 2.0)
    for q, a in enumerate(short_ids):
        if a not in long_ids:
            mem.append(a)
            h.append((0.0 - ws[q]) / 2.0)
    return np.asarray(mem, dtype=np.int64), np.asarray(h, dtype=np.float64)


def book(X, t, members, w, F, spec_t, fill_t, cov=True):
    """One book at date t -> dict(status (0 | 4), S [k][k] (or None), risk [4], contrib [K1])."""
    K1 = X.shape[0] + 1
    members = np.asarray(members, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    k = len(members)
    d = np.asarray(spec_t, dtype=np.float64)[members] if k else np.zeros(0)
    need = ~np.isfinite(d)
    bad = (not np.isfinite(F).all()) or (need.any() and not np.isfinite(fill_t))
    if bad:
        return dict(status=4, S=np.full((k, k), np.nan) if cov else None, risk=np.full(4, np.nan),
                    contrib=np.full(K1, np.nan))
    d = np.where(need, fill_t, d)
    B = exposures(X, t, members)
    x = np.zeros(K1)
    for m in range(k):
        x = x + B[m] * w[m]
    Fx = np.zeros(K1)
    for j in range(K1):
        Fx = Fx + F[:, j] * x[j]
    c = x * Fx
    fvar = 0.0
    for i in range(K1):
        fvar = fvar + c[i]
    svar = 0.0
    for m in range(k):
        svar = svar + (w[m] * w[m]) * d[m]
    S = None
    if cov:
        G = np.zeros((k, K1))
        for i in range(K1):
            G = G + B[:, i:i + 1] * F[i:i + 1, :]
        full = np.zeros((k, k))
        for j in range(K1):
            full = full + G[:, j:j + 1] * B[:, j][None, :]
        S = np.tril(full) + np.tril(full, -1).T                 # m >= n, mirrored
        S[np.arange(k), np.arange(k)] = S[np.arange(k), np.arange(k)] + d
    return dict(status=0, S=S, risk=np.array([fvar + svar, fvar, svar, float(need.sum())]),
                contrib=c)


def books(X, dates, k, book_ids, weights, fcov, spec, fill, kc):
    """afm_risk_book_f64 on host arrays -> (cov [nd][2][kc][kc] with NaN where nothing is written,
    risk [nd][3][4], contrib [nd][3][K1], status [nd])."""
    nd, K1 = len(dates), X.shape[0] + 1
    cov = np.full((nd, 2, kc, kc), np.nan)
    risk = np.full((nd, 3, 4), np.nan)
    contrib = np.full((nd, 3, K1), np.nan)
    status = np.zeros(nd, dtype=np.int32)
    for i, t in enumerate(dates):
        n = int(k[i])
        ids = [book_ids[i, s, :n] for s in (0, 1)]
        ws = [weights[i, s, :n] for s in (0, 1)]
        mem, h = net_book(ids[0], ws[0], ids[1], ws[1])
        for side, (mm, ww) in enumerate(((ids[0], ws[0]), (ids[1], ws[1]), (mem, h))):
            r = book(X, t, mm, ww, fcov[t], spec[t], fill[t], cov=side < 2)
            status[i] |= r["status"]
            risk[i, side], contrib[i, side] = r["risk"], r["contrib"]
            if side < 2:
                cov[i, side, :n, :n] = r["S"]
    return cov, risk, contrib, status


# ---- closed forms (longdouble), for tests/test_risk_ref.py ------------------------------------------
def factor_cov_closed(F, half_life, dtype=np.longdouble):
    """The weighted covariance of the rows of F (all used) with weights lambda^(n-1-s):
    sum w (f - mean)(f - mean)' / sum w, mean the weighted mean."""
    F = np.asarray(F, dtype=dtype)
    lam = dtype(0.5) ** (dtype(1.0) / dtype(half_life))
    w = lam ** np.arange(len(F) - 1, -1, -1, dtype=dtype)
    mean = (w[:, None] * F).sum(axis=0) / w.sum()
    Z = F - mean
    return (w[:, None, None] * Z[:, :, None] * Z[:, None, :]).sum(axis=0) / w.sum()


def specific_closed(u, half_life, dtype=np.longdouble):
    """sum w u^2 / sum w over one security's finite residuals, weights by observation count."""
    u = np.asarray(u, dtype=dtype)
    u = u[np.isfinite(u)]
    lam = dtype(0.5) ** (dtype(1.0) / dtype(half_life))
    w = lam ** np.arange(len(u) - 1, -1, -1, dtype=dtype)
    return (w * u * u).sum() / w.sum()
