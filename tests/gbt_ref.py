"""numpy restatement of the boosted-tree algorithm of include/afm_gbt.h -- the specification the
kernels of csrc/gbt.hip are held to bit for bit (trees, F, bins, histograms, predictions).

Fixed-point gradients make every histogram sum an exact integer, so nothing depends on the order
of addition; every floating-point step is one IEEE operation, written here in the order the
header states.
"""
import math

import numpy as np

LEAF, ABSENT = -1, -2


def make_cuts(X, w, B):
    """Per column: the distinct values among s[(j * m) // B], j = 1..B-1, of the sorted values s
    of the rows with w > 0 (-0.0 stored as 0.0).  Returns (cuts [p][B-1], zero padded; ncuts [p])."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    tr = np.asarray(w) > 0
    m = int(tr.sum())
    cuts = np.zeros((p, B - 1))
    ncuts = np.zeros(p, dtype=np.int32)
    pos = (np.arange(1, B, dtype=np.int64) * m) // B
    for k in range(p):
        s = np.sort(X[tr, k])
        c = np.unique(s[pos]) + 0.0
        ncuts[k] = len(c)
        cuts[k, :len(c)] = c
    return cuts, ncuts


def bin_matrix(X, cuts, ncuts):
    """uint8 [p][n_pad]: bin(x) = the number of cuts <= x; the padding rows hold 0."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    n_pad = (n + 63) // 64 * 64
    out = np.zeros((p, n_pad), dtype=np.uint8)
    for k in range(p):
        out[k, :n] = np.searchsorted(cuts[k, :ncuts[k]], X[:, k], side="right")
    return out


def histogram(bins, node, q, w, nnodes, B):
    """int64 [nnodes][p][B][2] = {sum q, sum w} of the rows of each node (node < 0: in none)."""
    p = bins.shape[0]
    n = len(node)
    h = np.zeros((nnodes, p, B, 2), dtype=np.int64)
    use = np.flatnonzero(np.asarray(node) >= 0)
    nd = np.asarray(node)[use]
    for k in range(p):
        b = bins[k, :n][use].astype(np.int64)
        np.add.at(h[:, k, :, 0], (nd, b), np.asarray(q, dtype=np.int64)[use])
        np.add.at(h[:, k, :, 1], (nd, b), np.asarray(w, dtype=np.int64)[use])
    return h


def scale_exponent(gmax, W):
    if gmax == 0:
        return 0
    return min(62 - int(W).bit_length() - math.frexp(gmax)[1], 960)


def quantize(F, y, w):
    """(q int64 [n], e): q = w * rint((F - y) * 2^e), 0 on the rows with w = 0."""
    g = F - y
    tr = w > 0
    e = scale_exponent(float(np.abs(g[tr]).max()), int(w.sum()))
    q = np.zeros(len(g), dtype=np.int64)
    q[tr] = w[tr].astype(np.int64) * np.rint(g[tr] * math.ldexp(1.0, e)).astype(np.int64)
    return q, e


def node_value(G, H, e, eta, lam):
    return eta * (-(np.float64(G) * math.ldexp(1.0, -e)) / (np.float64(H) + lam))


def best_split(hq, hw, G, H, ncuts, e, lam, gamma, mcw):
    """(gain, k, b, GL, HL) of the node's split, or None.  hq, hw: int64 [p][B]."""
    inv = math.ldexp(1.0, -e)
    g = np.float64(G) * inv
    gp = g * g / (np.float64(H) + lam)
    best = None
    with np.errstate(all="ignore"):
        for k in range(hq.shape[0]):
            nc = int(ncuts[k])
            if nc == 0:
                continue
            GL = np.cumsum(hq[k])[:nc]
            HL = np.cumsum(hw[k])[:nc]
            HR = H - HL
            gl = GL.astype(np.float64) * inv
            gr = (G - GL).astype(np.float64) * inv
            gain = gl * gl / (HL.astype(np.float64) + lam) + \
                gr * gr / (HR.astype(np.float64) + lam) - gp
            ok = (HL.astype(np.float64) >= mcw) & (HR.astype(np.float64) >= mcw) & (gain > gamma)
            if not ok.any():
                continue
            b = int(np.argmax(np.where(ok, gain, -np.inf)))
            if best is None or gain[b] > best[0]:
                best = (float(gain[b]), k, b, int(GL[b]), int(HL[b]))
    return best


def grow_tree(bins, q, w, e, cuts, ncuts, D, B, eta, lam, gamma, mcw):
    """One tree in heap order: (feat, bin, thr, val, leaf [n] = heap index of every row's leaf)."""
    n = len(q)
    nn = 2 ** (D + 1) - 1
    feat = np.full(nn, ABSENT, dtype=np.int32)
    sbin = np.full(nn, -1, dtype=np.int32)
    thr = np.zeros(nn)
    val = np.zeros(nn)
    stat = {0: (int(q.sum()), int(w.sum()))}
    feat[0] = LEAF
    val[0] = node_value(*stat[0], e, eta, lam)
    pos = np.zeros(n, dtype=np.int64)                  # heap index of the row's node
    for d in range(D):
        first = 2 ** d - 1
        local = np.where((pos >= first) & (feat[pos] != ABSENT), pos - first, -1)
        h = histogram(bins, local, q, w, 2 ** d, B)
        for j in range(2 ** d):
            v = first + j
            if feat[v] == ABSENT:
                continue
            G, H = stat[v]
            s = best_split(h[j, :, :, 0], h[j, :, :, 1], G, H, ncuts, e, lam, gamma, mcw)
            if s is None:
                continue
            _, k, b, GL, HL = s
            feat[v], sbin[v], thr[v] = k, b, cuts[k, b]
            for c, st in ((2 * v + 1, (GL, HL)), (2 * v + 2, (G - GL, H - HL))):
                stat[c] = st
                feat[c] = LEAF
                val[c] = node_value(*st, e, eta, lam)
            rows = np.flatnonzero(pos == v)
            pos[rows] = np.where(bins[k, :n][rows] <= b, 2 * v + 1, 2 * v + 2)
    return feat, sbin, thr, val, pos


def moment_terms(F, y):
    return [np.ones(len(F)), F, y, F * F, y * y, F * y]


def moments(F, y, w):
    """[2][6] = {count, sum F, sum y, sum F^2, sum y^2, sum F y} of the rows with w > 0 and with
    w = 0, each the correctly rounded sum (math.fsum)."""
    out = np.zeros((2, 6))
    for g, m in enumerate((w > 0, w == 0)):
        out[g] = [math.fsum(t) for t in moment_terms(F[m], y[m])]
    return out


def fit(X, y, w, *, n_rounds, max_depth=3, eta=0.025, reg_lambda=1.0, gamma=0.0,
        min_child_weight=1.0, max_bin=256, base_score=0.0):
    """The whole fit: dict of cuts, ncuts, bins, the trees feat / bin / thr / val [n_rounds][nn],
    F [n] (every row, w = 0 included), evals [n_rounds][2][6] and the exponents e [n_rounds]."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    w = np.asarray(w, dtype=np.int32)
    n = len(y)
    cuts, ncuts = make_cuts(X, w, max_bin)
    bins = bin_matrix(X, cuts, ncuts)
    nn = 2 ** (max_depth + 1) - 1
    out = {"cuts": cuts, "ncuts": ncuts, "bins": bins,
           "feat": np.zeros((n_rounds, nn), np.int32), "bin": np.zeros((n_rounds, nn), np.int32),
           "thr": np.zeros((n_rounds, nn)), "val": np.zeros((n_rounds, nn)),
           "evals": np.zeros((n_rounds, 2, 6)), "e": np.zeros(n_rounds, np.int64)}
    F = np.full(n, float(base_score))
    for r in range(n_rounds):
        q, e = quantize(F, y, w)
        feat, sbin, thr, val, leaf = grow_tree(bins, q, w, e, cuts, ncuts, max_depth, max_bin, eta,
                                               reg_lambda, gamma, min_child_weight)
        F = F + val[leaf]
        out["feat"][r], out["bin"][r], out["thr"][r], out["val"][r] = feat, sbin, thr, val
        out["evals"][r] = moments(F, y, w)
        out["e"][r] = e
    out["F"] = F
    return out


def predict(X, feat, thr, val, base_score=0.0, n_trees=None):
    """The tree walk over raw values: left iff x < thr; base_score plus one add per tree."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    s = np.full(n, float(base_score))
    rows = np.arange(n)
    for r in range(len(feat) if n_trees is None else n_trees):
        v = np.zeros(n, dtype=np.int64)
        while True:
            k = feat[r][v]
            go = k >= 0
            if not go.any():
                break
            x = X[rows[go], k[go]]
            v[go] = np.where(x < thr[r][v[go]], 2 * v[go] + 1, 2 * v[go] + 2)
        s = s + val[r][v]
    return s


def metrics(ev):
    """rmse and the Pearson IC of F against y from one group's six moments."""
    n, sf, sy, sff, syy, sfy = ev
    with np.errstate(all="ignore"):
        rmse = np.sqrt((sff - 2 * sfy + syy) / n)
        ic = (n * sfy - sf * sy) / np.sqrt((n * sff - sf * sf) * (n * syy - sy * sy))
    return rmse, ic
