"""The definitions of include/afm_turnover.h restated in numpy and Python integers: exact sums,
the stated add orders, float(int) conversions.  The yardstick of the GPU tests
(tests/test_turnover_kernels_gpu.py, tests/test_turnover_gpu.py); tests/test_turnover_ref.py holds
it against pandas.

``vals`` [K][T][lda]: the double the kernel reads for column k on date t and asset a (the raw
plane, or (x - mu) * (1/sd) computed in float64 one operation at a time).  ``rows_idx`` [T][lda],
``nrows`` [T]: the compacted asset indices of each date's rows; ``dates``: the evaluated dates,
paired by position."""
import math

import numpy as np

TOPK = 10
LAYERS = 10


def marks(v, idx):
    """One (date, column): ``v`` [lda] the date's values by asset, ``idx`` the date's rows (asset
    indices in row order).  Returns rank2 [lda] (Python-int doubled average ranks by asset, 0 = no
    rank), the asset sets of layer 10 and layer 1, the top book {asset: weight} and n_k."""
    v = np.asarray(v, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    rank2 = np.zeros(len(v), dtype=np.int64)
    idx = idx[~np.isnan(v[idx])]                           # the ranked rows, in row order
    x = v[idx]
    nk = len(x)
    if nk == 0:
        return [0] * len(v), set(), set(), {}, 0
    order = np.argsort(x, kind="stable")                   # -0.0 == 0.0; equal keys in row order
    xs = x[order]
    lb = np.searchsorted(xs, x, side="left")               # values below
    ub = np.searchsorted(xs, x, side="right")              # values up to
    earlier = np.empty(nk, dtype=np.int64)                 # equal values at earlier row positions
    earlier[order] = np.arange(nk) - lb[order]
    rank2[idx] = lb + ub + 1
    first = lb + 1 + earlier                               # rank(method='first'), ascending
    layer = np.minimum((first.astype(np.float64) / np.float64(nk) * LAYERS).astype(np.int64) + 1,
                       LAYERS)
    top = set(idx[layer == LAYERS].tolist())
    bot = set(idx[layer == 1].tolist())
    desc = (nk - ub) + 1 + earlier                         # rank(ascending=False, method='first')
    entries = sorted((int(d), int(a), float(f)) for d, a, f in zip(desc, idx, x) if d <= TOPK)
    rank2 = rank2.tolist()
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for _, _, x in entries:                            # in rank order 1, 2, ...
            total = total + np.float64(x)
        book ={a: np.float64(x) / total for _, a, x in entries}
    return rank2, top, bot, book, nk


def pair(m0, m1):
    """(rank_ac, [n, n_top, new_top, n_bot, new_bot], port_turn) of date t1 (``m1``) against the
    earlier date t0 (``m0``), each the result of ``marks``."""
    r0, top0, bot0, book0, _ = m0
    r1, top1, bot1, book1, _ = m1
    xy = [(x, y) for x, y in zip(r0, r1) if x > 0 and y > 0]
    n = len(xy)
    ac = math.nan
    if n >= 2:
        sx, sy = sum(x for x, _ in xy), sum(y for _, y in xy)
        cxy = n * sum(x * y for x, y in xy) - sx * sy
        cxx = n * sum(x * x for x, _ in xy) - sx * sx
        cyy = n * sum(y * y for _, y in xy) - sy * sy
        root = math.sqrt(float(cxx) * float(cyy))
        if root != 0:
            ac = float(cxy) / root
    counts = [n, len(top1), len(top1 - top0), len(bot1), len(bot1 - bot0)]
    turn = math.nan
    if book0 and book1 and all(math.isfinite(w) for w in list(book0.values()) +
                               list(book1.values())):
        s = np.float64(0.0)
        for a in sorted(set(book0) | set(book1)):
            s = s + abs(book1.get(a, np.float64(0.0)) - book0.get(a, np.float64(0.0)))
        turn = float(np.float64(0.5) * s)
    return ac, counts, turn


def turnover(vals, rows_idx, nrows, dates, lags):
    """rank_ac [nd][K][L], counts [nd][K][L][5] (int32), port_turn [nd][K][L]."""
    vals = np.asarray(vals, dtype=np.float64)
    K, nd, L = vals.shape[0], len(dates), len(lags)
    ac = np.full((nd, K, L), np.nan)
    counts = np.zeros((nd, K, L, 5), dtype=np.int32)
    turn = np.full((nd, K, L), np.nan)
    for k in range(K):
        mk = [marks(vals[k, t], rows_idx[t][:max(int(nrows[t]), 0)]) for t in dates]
        for i in range(nd):
            for l, lag in enumerate(lags):
                if i >= lag:
                    ac[i, k, l], counts[i, k, l], turn[i, k, l] = pair(mk[i - lag], mk[i])
    return ac, counts, turn


def summary(ac, counts, turn):
    """stats [K][L][4][2] = (n, mean) of rank_ac, new_top / n_top, new_bot / n_bot, port_turn over
    their non-NaN dates, summed in ascending position one add at a time."""
    nd, K, L = ac.shape
    stats = np.zeros((K, L, 4, 2))
    for k in range(K):
        for l in range(L):
            for s in range(4):
                total, n = np.float64(0.0), 0
                for i in range(nd):
                    if s == 0:
                        v = ac[i, k, l]
                    elif s == 3:
                        v = turn[i, k, l]
                    else:
                        den, num = counts[i, k, l, 2 * s - 1], counts[i, k, l, 2 * s]
                        v = np.float64(num) / np.float64(den) if den > 0 else np.nan
                    if not math.isnan(v):
                        total = total + np.float64(v)
                        n += 1
                stats[k, l, s] = (n, total / np.float64(n) if n else np.nan)
    return stats


def rows_of(mask):
    """mask [T][lda] bool -> (rows_idx [T][lda] int32, nrows [T] int32), assets ascending."""
    T, lda = mask.shape
    rows_idx = np.zeros((T, lda), dtype=np.int32)
    nrows = mask.sum(axis=1).astype(np.int32)
    for t in range(T):
        rows_idx[t, :nrows[t]] = np.flatnonzero(mask[t])
    return rows_idx, nrows
