"""numpy statements of include/afm_gbt_shap.h: the cover of every node, the TreeSHAP contributions
in the header's pinned order of operations (what the kernels of csrc/gbt_shap.hip are held to bit
for bit), the pinned aggregates, and -- independent of the per-path form -- the contributions by
the definition of the Shapley value, summed over subsets in np.longdouble.

The bound (``bound``), derived for the code as written, first order in u = 2^-53, for one cell and
one column.  A term is (val * (o_d - z_d)) * s_d with |o_d - z_d| <= 1 and 0 <= s_d <= 1 (the
W-weighted subset products: sum_k W[m][k] C(m-1, k) = 1, every product of z's and o's <= 1):

* the z's of the path: one division per split and one multiplication per split after an element's
  first, D + (D - m) <= 2D - 1 roundings; every z enters the term once (z_d in o_d - z_d, the
  others in the non-negative polynomial c), so they move it by at most (2D - 1) u |val|;
* the coefficients: at most m - 1 = 5 factors, each a multiplication by z and an addition (the
  multiplication by o is exact): 10; W[m][k] is a rounded quotient and c[k] * W[m][k] a rounded
  product: 2; the k-sum m - 1 = 5 additions: 17 in all, every quantity non-negative;
* o_d - z_d, val * (.), (.) * s_d: 3.

So a term is off by at most (2D + 19) u |val| (the issue's count, 4D + 24, allows two roundings
per z operation and five outer ones; the code has one and three).  The bias term val * (z_0 * ..)
has at most 3D roundings, fewer.  The running sum of a column takes at most n_trees * 2^D
additions, each off by at most u times the partial sum, itself at most S = |base_score| + the sum
of |val| over the leaves of the trees used.  Together

    E = (n_trees * 2^D + 2D + 19) * u * S,

and the tests allow 2E for the second-order terms.  The comparison is always against
``contribs_by_definition``, never against the kernel.
"""
import itertools
import math

import numpy as np

LEAF, ABSENT = -1, -2
U = 2.0 ** -53


def depth_of(feat):
    return int(np.log2(np.asarray(feat).shape[-1] + 1)) - 1


def cover(bins, w, feat, sbin):
    """int64 [n_trees][nn]: the sum of w over the rows that reach each node; a row moves right iff
    bins[feat[v]][i] > bin[v].  w <= 0 counts as 0."""
    feat, sbin = np.asarray(feat), np.asarray(sbin)
    w = np.maximum(np.asarray(w, dtype=np.int64), 0)
    n = len(w)
    R, nn = feat.shape
    p = bins.shape[0]
    out = np.zeros((R, nn), dtype=np.int64)
    rows = np.arange(n)
    for r in range(R):
        v = np.zeros(n, dtype=np.int64)
        np.add.at(out[r], v, w)
        while True:
            k = feat[r][v]
            go = (k >= 0) & (k < p) & (2 * v + 2 < nn)
            if not go.any():
                break
            b = bins[k[go], rows[go]].astype(np.int64)
            v[go] = 2 * v[go] + 1 + (b > sbin[r][v[go]])
            np.add.at(out[r], v[go], w[go])
    return out


def paths(feat_r, cover_r):
    """The leaves of one tree in heap order: (leaf, cols, z, splits) with splits[j] = the
    (node, goes_left) pairs of element j, merged by column in order of first appearance."""
    out = []
    for v in range(len(feat_r)):
        if feat_r[v] != LEAF:
            continue
        dep = (v + 1).bit_length() - 1
        cols, z, splits = [], [], []
        for s in range(dep, 0, -1):
            a, c = ((v + 1) >> s) - 1, ((v + 1) >> (s - 1)) - 1
            k = int(feat_r[a])
            assert k >= 0
            with np.errstate(all="ignore"):
                ratio = np.float64(cover_r[c]) / np.float64(cover_r[a])
            if k in cols:
                j = cols.index(k)
                z[j] = z[j] * ratio
            else:
                j = len(cols)
                cols.append(k)
                z.append(ratio)
                splits.append([])
            splits[j].append((a, c == 2 * a + 1))
        out.append((v, cols, z, splits))
    return out


def weight(m, k):
    return np.float64(math.factorial(k) * math.factorial(m - 1 - k)) / \
        np.float64(math.factorial(m))


def contribs_pinned(X, feat, thr, val, cov, base_score=0.0, n_trees=None):
    """float64 [n][p+1], the bias last: the header's operations in the header's order."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    phi = np.zeros((n, p + 1))
    phi[:, p] = np.float64(base_score)
    with np.errstate(all="ignore"):
        for r in range(len(feat) if n_trees is None else n_trees):
            for v, cols, z, splits in paths(feat[r], cov[r]):
                m = len(cols)
                vl = np.float64(val[r][v])
                if m == 0:
                    phi[:, p] = phi[:, p] + vl
                    continue
                o = []
                for j in range(m):
                    ok = np.ones(n, dtype=bool)
                    for a, left in splits[j]:
                        ok &= (X[:, cols[j]] < thr[r][a]) == left
                    o.append(np.where(ok, 1.0, 0.0))
                for d in range(m):
                    c = [np.ones(n)]
                    for j in range(m):
                        if j == d:
                            continue
                        nc = len(c)
                        new = [None] * (nc + 1)
                        new[nc] = c[nc - 1] * o[j]
                        for k in range(nc - 1, 0, -1):
                            new[k] = c[k] * z[j] + c[k - 1] * o[j]
                        new[0] = c[0] * z[j]
                        c = new
                    s = c[0] * weight(m, 0)
                    for k in range(1, m):
                        s = s + c[k] * weight(m, k)
                    phi[:, cols[d]] = phi[:, cols[d]] + (vl * (o[d] - z[d])) * s
                P = z[0]
                for j in range(1, m):
                    P = P * z[j]
                phi[:, p] = phi[:, p] + vl * P
    return phi


def agg_pinned(contrib, use):
    """contrib [nt][p+1][lda], use bool [nt][lda] -> (agg [nt][p+1][2] = {sum phi, sum |phi|} in
    the header's order: the 64-asset tree, +0.0 for unset cells, then the blocks ascending;
    cnt int64 [nt])."""
    contrib = np.asarray(contrib, dtype=np.float64)
    nt, pc, lda = contrib.shape
    agg = np.zeros((nt, pc, 2))
    x = np.where(use[:, None, :], contrib, 0.0)
    for which, s in enumerate((x, np.abs(x))):
        s = s.reshape(nt, pc, lda // 64, 64).copy()
        st = 32
        while st:
            s[..., :st] = s[..., :st] + s[..., st:2 * st]
            st //= 2
        tot = s[..., 0, 0].copy()
        for b in range(1, lda // 64):
            tot = tot + s[..., b, 0]
        agg[..., which] = tot
    return agg, use.sum(axis=1).astype(np.int64)


def _expect(feat_r, thr_r, val_r, cov_r, X, S, v=0):
    """E[f | x_S] of one tree by recursion, longdouble [n]: follow the split if its column is in
    S, else the cover-weighted mean of the children."""
    k = int(feat_r[v])
    if k < 0:
        return np.full(X.shape[0], np.longdouble(val_r[v]))
    L = _expect(feat_r, thr_r, val_r, cov_r, X, S, 2 * v + 1)
    Rt = _expect(feat_r, thr_r, val_r, cov_r, X, S, 2 * v + 2)
    if k in S:
        return np.where(X[:, k] < thr_r[v], L, Rt)
    cl, cr = np.longdouble(cov_r[2 * v + 1]), np.longdouble(cov_r[2 * v + 2])
    return (cl * L + cr * Rt) / np.longdouble(cov_r[v])


def _reachable(feat_r):
    out, todo = [], [0]
    while todo:
        v = todo.pop()
        out.append(v)
        if feat_r[v] >= 0:
            todo += [2 * v + 1, 2 * v + 2]
    return out


def contribs_by_definition(X, feat, thr, val, cov, base_score=0.0, n_trees=None):
    """longdouble [n][p+1]: per tree the Shapley values of the game v(S) = E[f | x_S] over the
    columns the tree uses, every subset enumerated; the bias is v(empty) summed, plus base_score."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    phi = np.zeros((n, p + 1), dtype=np.longdouble)
    phi[:, p] = np.longdouble(base_score)
    for r in range(len(feat) if n_trees is None else n_trees):
        used = sorted({int(feat[r][v]) for v in _reachable(feat[r]) if feat[r][v] >= 0})
        M = len(used)
        assert M <= 12, "too many columns for the enumeration"
        value = {}
        for size in range(M + 1):
            for S in itertools.combinations(used, size):
                value[S] = _expect(feat[r], thr[r], val[r], cov[r], X, set(S))
        phi[:, p] += value[()]
        for i in used:
            rest = [k for k in used if k != i]
            for size in range(M):
                wt = (np.longdouble(math.factorial(size) * math.factorial(M - 1 - size)) /
                      np.longdouble(math.factorial(M)))
                for S in itertools.combinations(rest, size):
                    phi[:, i] += wt * (value[tuple(sorted(S + (i,)))] - value[S])
    return phi


def bound(feat, val, base_score=0.0, n_trees=None):
    """E of the module docstring for these trees (a scalar: it holds for every cell and column)."""
    R = len(feat) if n_trees is None else n_trees
    D = depth_of(feat)
    S = abs(float(base_score)) + float(np.abs(np.asarray(val)[:R][np.asarray(feat)[:R] == LEAF]).sum())
    return (R * 2 ** D + 2 * D + 19) * U * S


def random_trees(rng, R, D, p, ncols=6, n_rows=4096, leaf_p=0.25, grid=None):
    """R random trees of depth <= D on at most ``ncols`` of p columns, with covers that are the
    counts of ``n_rows`` random rows (so every present node has cover >= 1 and a split's cover is
    the sum of its children's).  Returns feat, thr, val, cover and the rows' matrix."""
    nn = 2 ** (D + 1) - 1
    pool = rng.choice(p, size=min(ncols, p), replace=False)
    Xc = np.round(rng.standard_normal((n_rows, p)) * 4) / 4
    feat = np.full((R, nn), ABSENT, dtype=np.int32)
    thr = np.zeros((R, nn))
    val = np.zeros((R, nn))
    cov = np.zeros((R, nn), dtype=np.int64)
    for r in range(R):
        members = {0: np.arange(n_rows)}
        for v in range(nn):
            if v not in members:
                continue
            rows = members[v]
            cov[r, v] = len(rows)
            val[r, v] = (np.round(rng.standard_normal() * 8) / 8 if grid else
                         rng.standard_normal() * 0.05)
            feat[r, v] = LEAF
            if 2 * v + 2 >= nn or (v > 0 and rng.random() < leaf_p):
                continue
            for _ in range(8):
                k = int(rng.choice(pool))
                t = float(rng.choice(Xc[rows, k]))
                left = Xc[rows, k] < t
                if left.any() and not left.all():
                    feat[r, v], thr[r, v] = k, t
                    members[2 * v + 1], members[2 * v + 2] = rows[left], rows[~left]
                    break
    return feat, thr, val, cov, Xc
