"""Reference of the mean-variance rebalance (test infrastructure only, no GPU).

    minimise  1/2 w'S w - gamma * s * mu'w     s.t.  sum w = 1,  lo <= w <= hi

``box_qp_mv`` is oracle.portfolio.box_qp_weights (exact primal active set, Cholesky refactored at
every step) with the linear term in the step's right-hand side and in the multipliers, and with an
optimality test at the fully bound vertex; ``kkt_residual`` checks a weight vector without any
solver; ``run_portfolio_mv`` is oracle.portfolio.run_portfolio with that solve.  The sign ``s`` of
the short book is folded into ``mu`` by the caller.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle.portfolio import _value_recursion, book_history, pairwise_cov, select_books
from oracle.xs import np_sum


def box_qp_mv(S, mu, gamma: float, lo: float = 0.0, hi: float = 0.1, max_iter: int = 0):
    """Returns (w, iterations).  ``mu`` non-finite counts as 0."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    if n == 0:
        return np.zeros(0), 0
    if n * hi <= 1.0:
        return np.full(n, hi), 0
    if n * lo >= 1.0:
        return np.full(n, lo), 0
    mu = np.asarray(mu, dtype=np.float64)
    gm = gamma * np.where(np.isfinite(mu), mu, 0.0)
    max_iter = max_iter or 4 * n + 8
    w = np.full(n, 1.0 / n)
    state = np.zeros(n, dtype=np.int8)          # 0 free, -1 at lo, +1 at hi
    it = 0
    while it < max_iter:
        it += 1
        F = np.flatnonzero(state == 0)
        B = np.flatnonzero(state != 0)
        b = 1.0 - w[B].sum()
        if len(F) == 0:
            # fully bound vertex: move mass from the hi member with the largest gradient to the
            # lo member with the smallest one, if that descends (ties: ascending index)
            g = S @ w - gm
            H, Lo = np.flatnonzero(state == 1), np.flatnonzero(state == -1)
            if len(H) == 0 or len(Lo) == 0:
                break
            i = H[int(np.argmax(g[H]))]
            j = Lo[int(np.argmin(g[Lo]))]
            if not g[i] > g[j]:
                break
            state[i] = 0
            state[j] = 0
            continue
        SFF = S[np.ix_(F, F)]
        c = (S[np.ix_(F, B)] @ w[B] if len(B) else np.zeros(len(F))) - gm[F]
        L = np.linalg.cholesky(SFF)
        y1 = np.linalg.solve(L.T, np.linalg.solve(L, np.ones(len(F))))
        y2 = np.linalg.solve(L.T, np.linalg.solve(L, c))
        lam = -(b + y2.sum()) / y1.sum()
        x = -y2 - lam * y1
        if np.all(x >= lo) and np.all(x <= hi):
            w[F] = x
            g = S @ w - gm + lam
            viol = np.where(state == -1, g, np.where(state == 1, -g, np.inf))
            j = int(np.argmin(viol))
            if viol[j] >= 0:
                break
            state[j] = 0
            continue
        p = x - w[F]
        alpha, jb, bound = 1.0, -1, 0
        for k, i in enumerate(F):
            if x[k] < lo and p[k] < 0:
                a = (lo - w[i]) / p[k]
                if a < alpha:
                    alpha, jb, bound = a, i, -1
            elif x[k] > hi and p[k] > 0:
                a = (hi - w[i]) / p[k]
                if a < alpha:
                    alpha, jb, bound = a, i, 1
        w[F] = w[F] + alpha * p
        if jb >= 0:
            w[jb] = lo if bound < 0 else hi
            state[jb] = bound
    return w, it


def kkt_residual(S, mu, gamma: float, w, lo: float = 0.0, hi: float = 0.1, slack: float = 1e-14):
    """Largest violation of the KKT conditions of ``w`` relative to max|g|, g = S w - gamma mu.
    Members within ``slack`` of a bound count as bound."""
    S = np.asarray(S, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    g = S @ w - gamma * np.where(np.isfinite(mu), mu, 0.0)
    at_lo = w <= lo + slack
    at_hi = (w >= hi - slack) & ~at_lo
    free = ~at_lo & ~at_hi
    if free.any():
        lam = -g[free].mean()
    else:
        top = g[at_hi].max() if at_hi.any() else g[at_lo].min()
        bot = g[at_lo].min() if at_lo.any() else top
        lam = -0.5 * (top + bot)
    r = g + lam
    res = 0.0
    if free.any():
        res = max(res, np.abs(r[free]).max())
    if at_lo.any():
        res = max(res, (-r[at_lo]).max())
    if at_hi.any():
        res = max(res, r[at_hi].max())
    return res / np.abs(g).max()


def history_mean(R):
    """Column means over the finite rows (the reference's ``returns.mean()``, KKT:821)."""
    R = np.asarray(R, dtype=np.float64)
    fin = np.isfinite(R)
    n = fin.sum(axis=0)
    s = np.where(fin, R, 0.0).sum(axis=0)
    return np.where(n > 0, s / np.maximum(n, 1), 0.0)


def make_book(rng, k: int, rows: int, holes: bool):
    """A book's history returns: N(0, 0.02) * U(0.5, 2) per column plus a 1 % common factor."""
    R = rng.normal(0, 0.02, (rows, k)) * rng.uniform(0.5, 2, k) + rng.normal(0, 0.01, (rows, 1))
    if holes:
        R[rng.random(R.shape) < 0.02] = np.nan
    return R


def book_bounds(k: int):
    return 0.0, (max(0.1, 2.0 / k) if k < 20 else 0.1)


GAMMAS = (0.0, 0.02, 0.2, 5.0)


def ambiguous_bounds(w, lo: float, hi: float, slack: float = 1e-14, tol: float = 1e-9):
    """True if a weight lies within the weight tolerance of a bound without being at it (within
    ``slack``): the bound sets of two solves that agree to ``tol`` are then not comparable.  It
    happens at a degenerate vertex (k = 2 with hi = 1: one name at hi forces the other to lo), where
    the last free member's x = -y2 - lam y1 cancels to a few ulp of y2, not of the weight."""
    dlo, dhi = np.asarray(w) - lo, hi - np.asarray(w)
    return bool((((dlo > slack) & (dlo < tol)) | ((dhi > slack) & (dhi < tol))).any())


# the grid's seed: the smallest from 7 on at which no reference solution is ambiguous in that
# sense (tests/test_mv_ref.py asserts it; at 7 one book of two names is, at risk tolerance 5)
GRID_SEED = 8


@functools.lru_cache(maxsize=None)
def book_grid(k: int, seed: int = GRID_SEED):
    """The books of k names of the issue's grid: rows in (2k + 8, 300), without / with 2 % holes,
    ``mu`` the history mean (source "history") or N(0, 1e-3) (source "given"); each solved by
    ``box_qp_mv`` at every tolerance of GAMMAS.  A list of dicts (k, rows, holes, source, R, mu,
    lo, hi, S, sol = {gamma: (w, iterations)}), computed once per session and shared: read only."""
    rng = np.random.default_rng([seed, k])
    lo, hi = book_bounds(k)
    out = []
    for rows in (2 * k + 8, 300):
        for holes in (False, True):
            R = make_book(rng, k, rows, holes)
            S = pairwise_cov(R)
            for source, mu in (("history", history_mean(R)), ("given", rng.normal(0, 1e-3, k))):
                sol = {g: box_qp_mv(S, mu, g, lo, hi) for g in GAMMAS}
                out.append(dict(k=k, rows=rows, holes=holes, source=source, R=R, mu=mu, lo=lo,
                                hi=hi, S=S, sol=sol))
    return out


def run_portfolio_mv(pred_date, pred_id, pred, hist_date, hist_id, hist, all_date, all_id,
                     all_tradable, all_close, all_tmr, trading_cost_rate=1e-4, top_n=10,
                     window=None, lo=0.0, hi=0.1, gamma=0.0, expected="prediction"):
    """oracle.portfolio.run_portfolio with the mean-variance solve.  ``expected``: "prediction"
    (mu = the date's predictions of the members) or "history" (the members' window means).  The
    short book solves with -mu."""
    akey = {(d, i): j for j, (d, i) in enumerate(zip(all_date.tolist(), all_id.tolist()))}
    udates = np.unique(pred_date)
    calendar = np.unique(np.concatenate([pred_date, hist_date, all_date]))
    recs = []
    for dt in udates:
        m = pred_date == dt
        ids, vals = pred_id[m], pred[m]
        rows = np.array([akey.get((dt, i), -1) for i in ids.tolist()])
        trad = np.array([r >= 0 and bool(all_tradable[r]) for r in rows])
        pmap = dict(zip(ids.tolist(), vals.tolist()))
        ws = []
        books = select_books(ids, vals, trad, top_n)
        for sign, book in zip((1.0, -1.0), books):
            R = book_history(hist_date, hist_id, hist, book, window, dt, calendar)
            mu = history_mean(R) if expected == "history" else \
                np.array([pmap[x] for x in book.tolist()])
            ws.append(box_qp_mv(pairwise_cov(R), sign * mu, gamma, lo, hi)[0])
        L, S = books
        wl, wsh = ws
        rl = np.array([all_tmr[akey[(dt, i)]] for i in L.tolist()])
        rs = np.array([all_tmr[akey[(dt, i)]] for i in S.tolist()])
        pl = np.array([all_close[akey[(dt, i)]] for i in L.tolist()])
        ps = np.array([all_close[akey[(dt, i)]] for i in S.tolist()])
        lsum, ssum = np_sum(np.nan_to_num(rl * wl)), np_sum(np.nan_to_num(rs * wsh))
        den_l = 0
        for x in (wl * pl).tolist():
            den_l = den_l + x
        den_s = 0
        for x in (wsh * ps).tolist():
            den_s = den_s + x
        recs.append(dict(ids=ids, L=L, S=S, wl=wl, ws=wsh, lsum=lsum, ssum=ssum, den_l=den_l,
                         den_s=den_s))
    res = _value_recursion(recs, trading_cost_rate)
    res["books"] = [x for b in recs for x in (b["L"], b["S"])]
    res["weights"] = [x for b in recs for x in (b["wl"], b["ws"])]
    res["dates"] = udates
    return res
