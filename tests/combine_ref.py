"""numpy restatement of include/afm_combine.h: the rolling IC weights (afm_ic_weights_f64) and the
weighted composite (afm_combine_f64), each generic in the dtype: np.float64 with the stated orders
-- every sum in ascending j (the window) or ascending k (the normalisation and the composite), one
add per term from 0.0, which the engine must match bit for bit for methods 0..2 and the composite
-- and np.longdouble, the yardstick of method 3 (no linalg there: the Cholesky is written out).
tests/test_combine_ref.py pins this file against pandas and numpy.linalg."""
import numpy as np

EQUAL, IC, ICIR, MAXIR = 0, 1, 2, 3
U = 2.0 ** -53


def window_of(i, window, embargo):
    """The positions J of row i (empty where i < embargo)."""
    j1 = i - embargo
    if j1 < 0:
        return range(0)
    return range(max(0, j1 - window + 1), j1 + 1)


def _cholesky_solve(A, b):
    """x with A x = b by Cholesky in A's dtype; None when a pivot is not > 0."""
    n = len(b)
    L = A.copy()
    for p in range(n):
        d = L[p, p]
        if not d > 0:
            return None
        L[p, p] = np.sqrt(d)
        L[p + 1:, p] = L[p + 1:, p] / L[p, p]
        c = L[p + 1:, p]                                   # (the upper triangle is not read)
        L[p + 1:, p + 1:] = L[p + 1:, p + 1:] - np.outer(c, c)
    y = b.copy()
    for p in range(n):
        y[p] = y[p] / L[p, p]
        y[p + 1:] = y[p + 1:] - L[p + 1:, p] * y[p]
    for p in range(n - 1, -1, -1):
        y[p] = y[p] / L[p, p]
        y[:p] = y[:p] - L[p, :p] * y[p]
    return y


def maxir_system(icq, J, min_periods, shrink, dtype):
    """(active columns, D, A, m) of method 3 for the window J of icq [nd][K]: A, m in ``dtype``
    over the active columns (None, None without one)."""
    K = icq.shape[1]
    J = np.asarray(list(J), dtype=np.int64)
    win = icq[J] if len(J) else np.zeros((0, K))
    fin = np.isfinite(win)
    cand = np.flatnonzero(fin.sum(axis=0) >= min_periods)
    D = J[fin[:, cand].all(axis=1)] if len(J) else J
    if len(D) < min_periods or not len(cand):
        return np.zeros(0, dtype=np.int64), D, None, None
    X = icq[D][:, cand].astype(dtype)
    n = dtype(len(D))
    s = np.zeros(len(cand), dtype=dtype)
    for row in X:                                          # ascending j
        s = s + row
    m = s / n
    C = X - m
    ss = np.zeros(len(cand), dtype=dtype)
    for row in C:
        ss = ss + row * row
    keep = ss / (n - dtype(1)) > 0
    act = cand[keep]
    if not len(act):
        return act, D, None, None
    C, m = C[:, keep], m[keep]
    S = np.zeros((len(act), len(act)), dtype=dtype)
    for row in C:
        S = S + np.outer(row, row)
    S = S / (n - dtype(1))
    sh = dtype(shrink)
    A = (dtype(1) - sh) * S
    A[np.diag_indices(len(act))] = (dtype(1) - sh) * np.diag(S) + sh * np.diag(S)
    return act, D, A, m


def ic_weights_ref(ic, q, method, window, embargo, min_periods, shrink=0.5, dtype=np.float64,
                   systems=None, raws=None):
    """w [nd][K], info [nd][3] of afm_ic_weights_f64 in ``dtype``.  ``systems``: a list that
    receives (i, active, D, A, m, raw) of every position of method 3; ``raws``: a list that
    receives (raw [K], active [K]) of every position."""
    ic = np.asarray(ic, dtype=np.float64)
    nd, K = ic.shape[0], ic.shape[1]
    icq = ic[:, :, q]
    w = np.full((nd, K), np.nan, dtype=dtype)
    info = np.zeros((nd, 3), dtype=dtype)
    for i in range(nd):
        J = window_of(i, window, embargo)
        raw = np.zeros(K, dtype=dtype)
        act = np.zeros(K, dtype=bool)
        n_dates, fail = 0, False
        if method == EQUAL:
            raw[:] = 1
            act[:] = True
        elif method in (IC, ICIR):
            s = np.zeros(K, dtype=dtype)
            n = np.zeros(K, dtype=np.int64)
            for j in J:                                    # ascending j, one add per term
                v = icq[j].astype(dtype)
                f = np.isfinite(v)
                s = np.where(f, s + np.where(f, v, 0), s)
                n += f
            n_dates = int(n.max())
            ok = n >= min_periods
            with np.errstate(all="ignore"):
                m = s / n.astype(dtype)
                if method == IC:
                    act, raw = ok, np.where(ok, m, 0)
                else:
                    ss = np.zeros(K, dtype=dtype)
                    for j in J:
                        v = icq[j].astype(dtype)
                        f = np.isfinite(v)
                        d = np.where(f, v, 0) - m
                        ss = np.where(f, ss + d * d, ss)
                    sd = np.sqrt(ss / (n - 1).astype(dtype))
                    act = ok & np.isfinite(sd) & (sd > 0)
                    raw = np.where(act, m / np.where(act, sd, 1), 0)
        elif method == MAXIR:
            a, D, A, m = maxir_system(icq, J, min_periods, shrink, dtype)
            n_dates = len(D)
            x = None
            if len(a):
                x = _cholesky_solve(A, m)
                fail = x is None
                if not fail:
                    act[a] = True
                    raw[a] = x
                else:
                    act[a] = True
            if systems is not None:
                systems.append((i, a, D, A, m, x))
        else:
            raise ValueError(method)
        if raws is not None:
            raws.append((raw.copy(), act.copy()))
        total = dtype(0)
        for k in range(K):                                 # ascending k
            if act[k]:
                total = total + abs(raw[k])
        if fail:
            total = dtype(np.nan)
        info[i] = (act.sum(), n_dates, total)
        if act.any() and np.isfinite(total) and total > 0:
            w[i] = np.where(act, raw / total, 0)
    return w, info


def combine_ref(base, cols, dates, rows_idx, nrows, w, out, cnt, zs=None, zcols=None,
                dtype=np.float64):
    """afm_combine_f64 on host arrays: base [P][T][lda], w [nd][K] or [K]; writes into copies of
    ``out`` [T][lda] / ``cnt`` [T][lda] (the sentinels of the dates that are not evaluated stay)
    and returns them."""
    base = np.asarray(base, dtype=np.float64)
    T, lda = base.shape[1], base.shape[2]
    out = np.array(out, dtype=dtype)
    cnt = np.array(cnt, dtype=np.int32)
    w = np.asarray(w, dtype=np.float64)
    K = len(cols)
    for i, t in enumerate(dates):
        wi = w if w.ndim == 1 else w[i]
        n = min(max(int(nrows[t]), 0), lda)
        a = np.asarray(rows_idx[t][:n], dtype=np.int64)
        num = np.zeros(n, dtype=dtype)
        den = np.zeros(n, dtype=dtype)
        c = np.zeros(n, dtype=np.int32)
        for k in range(K):                                 # ascending k
            wk = wi[k]
            if not np.isfinite(wk) or wk == 0:
                continue
            x = base[cols[k], t, a]
            with np.errstate(all="ignore"):
                if zs is not None:
                    zr = zcols[k] if zcols is not None else k
                    x = (x - zs[zr, a, 0]) * zs[zr, a, 1]
                f = np.isfinite(x)
                pr = dtype(wk) * np.where(f, x, 0).astype(dtype)   # one rounded multiply
                num = np.where(f, num + pr, num)                   # then one add
                den = np.where(f, den + dtype(abs(wk)), den)
            c += f
        out[t, :] = np.nan
        cnt[t, :] = 0
        with np.errstate(all="ignore"):
            out[t, a] = np.where(c > 0, num / np.where(c > 0, den, 1), np.nan)
        cnt[t, a] = c
    return out, cnt
