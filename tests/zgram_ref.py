"""Host reference and poisoned panels for the direct tests of the Gram kernels (afm_zgram_f64,
afm_zpool_f64) and of afm_zpredict_f64 (test infrastructure, CPU only):
tests/test_zgram_edges_gpu.py, tests/test_zpredict_gpu.py and their CPU checks in
tests/test_zgram_ref.py.

The Gram of one item is G = D D^T over the item's rows, D = [1, z_1..z_p, y] with z = (x - mu) * rs
as two separately rounded fp64 operations (the kernels' z; the library is built without FMA
contraction) or the raw columns.  ``gram_exact`` accumulates it in ``np.longdouble`` together with
the magnitudes M = |D| |D|^T.  Any summation order of n fp64 products is within gamma_n * M of G,
gamma_n = n u / (1 - n u), u = 2^-53, so the GPU tests accept ``bound(n, M) = 2 n u M`` entry by
entry -- derived, not measured; a dropped or doubled row moves an entry by about M / n.

``make_panel``: the one small panel every GPU test shares.  Its row set is the cells with the
presence bit set, a < A_END and a date in [T0, T0 + NT); every other cell of every plane is poisoned
(NaN, +inf, -inf, 1e308 in rotation), presence bits are set at random outside the row set too, the
two unused planes are all NaN and the statistics of assets without a row are NaN.  ``kind="int"``
draws x, y in [-8, 8], mu in [-2, 2], rs in {0.5, 1, 2}: every z, product and partial sum is exactly
representable, so the expected Gram comes from int64 arithmetic and must match bit for bit.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
T, LDA, A_END = 70, 192, 150            # dates, padded assets (3 row-blocks), assets present
T0, NT = 29, 37                         # dates 29..65: cross bit 32 and bit 64 of the words
EMPTY_DATE, EMPTY_ASSET = 40, 70        # a date and an asset column without rows
POISON = np.array([np.nan, np.inf, -np.inf, 1e308])


def pack_words(keep):
    """keep [T][lda] bool -> presence words uint64 [ceil(T / 64)][lda]: bit t % 64 of word t // 64"""
    keep = np.asarray(keep, dtype=bool)
    w = np.zeros(((keep.shape[0] + 63) // 64, keep.shape[1]), np.uint64)
    for t in range(keep.shape[0]):
        w[t // 64] |= keep[t].astype(np.uint64) << np.uint64(t % 64)
    return w


def poison_cells(plane, where, phase=0):
    """plane[where] = NaN, +inf, -inf, 1e308 in rotation (starting at ``phase``)."""
    idx = np.flatnonzero(where)
    plane.reshape(-1)[idx] = POISON[(np.arange(len(idx)) + phase) % 4]


# ---- the design and its Gram ---------------------------------------------------------------------
def design(x, y, mu=None, rs=None):
    """x [p][n], y [n] (and mu, rs [p][n]) -> D [p+2][n] = [1, z, y]; mu None: the raw columns."""
    x = np.asarray(x, dtype=np.float64)
    z = x if mu is None else (x - mu) * rs           # two roundings, as the kernels stage it
    return np.concatenate([np.ones((1, x.shape[1])), z, np.asarray(y, dtype=np.float64)[None]])


def gram_exact(D):
    """-> (G, M, n): G = D D^T and M = |D| |D|^T accumulated in longdouble, n rows."""
    Dl = np.asarray(D, dtype=np.float64).astype(LD)
    A = np.abs(Dl)
    return Dl @ Dl.T, A @ A.T, D.shape[1]


def gram_f64(D):
    """numpy's own fp64 D D^T."""
    D = np.asarray(D, dtype=np.float64)
    return D @ D.T


def gram_int4(D):
    """4 D D^T in int64 for a design on the half-integer grid (exact)."""
    D2 = np.rint(2.0 * D).astype(np.int64)
    assert np.array_equal(D2, 2.0 * D), "design is not on the half-integer grid"
    return D2 @ D2.T


def bound(n, M):
    """The component-wise error bound of an fp64 Gram of n rows: 2 n 2^-53 M (n at least 1)."""
    return 2 * max(int(n), 1) * LD(U) * M


# ---- the shared panel ----------------------------------------------------------------------------
class Panel:
    """planes [p+3][T][LDA], cols [p], ycol, zs [p+1][LDA][2] (row p: the identity row), keep (the
    presence bits as passed), rows (the row set), words."""

    def __init__(self, p, kind, seed):
        rng = np.random.default_rng([seed, p, kind == "int"])
        self.p, self.kind = p, kind
        ncol = p + 3                                           # p features + y + 2 unused
        perm = rng.permutation(ncol)
        self.cols, self.ycol = perm[:p].astype(np.int32), int(perm[p])
        if kind == "int":
            planes = rng.integers(-8, 9, size=(ncol, T, LDA)).astype(np.float64)
            mu = rng.integers(-2, 3, size=(p, LDA)).astype(np.float64)
            rs = rng.choice([0.5, 1.0, 2.0], size=(p, LDA))
        else:
            # features scattered around their own statistics (z-scores are centred with unit
            # spread by construction); the regressand is a return-like column
            mu = rng.normal(4.0, 3.0, size=(p, LDA))
            sd = rng.uniform(0.5, 20.0, size=(p, LDA))
            rs = 1.0 / sd
            planes = rng.normal(0.5, 2.0, size=(ncol, T, LDA))
            planes[perm[:p]] = mu[:, None, :] + sd[:, None, :] * rng.normal(size=(p, T, LDA))
        keep = rng.random((T, LDA)) < 0.8
        keep[EMPTY_DATE] = False
        keep[:, EMPTY_ASSET] = False
        rows = keep.copy()
        rows[:, A_END:] = False
        rows[:T0] = False
        rows[T0 + NT:] = False
        for k in range(ncol):
            poison_cells(planes[k], ~rows, phase=k)
        planes[perm[p + 1:]] = np.nan                          # the unused planes
        zs = np.zeros((p + 1, LDA, 2))
        zs[:p, :, 0], zs[:p, :, 1] = mu, rs
        zs[p, :, 1] = 1.0                                      # identity row: y passes unchanged
        zs[:, ~rows.any(axis=0)] = np.nan                      # assets without a row
        self.planes, self.zs, self.keep, self.rows = planes, zs, keep, rows
        self.words = pack_words(keep)
        self._groups = {}

    def design(self, tt, aa, raw=False):
        """D [p+2][n] of the cells (tt[i], aa[i])."""
        p = self.p
        x = np.stack([self.planes[c][tt, aa] for c in self.cols]).reshape(p, len(aa))
        y = self.planes[self.ycol][tt, aa]
        if raw:
            return design(x, y)
        y = (y - self.zs[p, aa, 0]) * self.zs[p, aa, 1]         # the identity row {0, 1}: exact
        return design(x, y, self.zs[:p, aa, 0], self.zs[:p, aa, 1])

    def zplanes(self):
        """[p+1][T][LDA]: the host-computed (x - mu) * rs of every feature, then y; poisoned
        outside the row set like the planes themselves."""
        p = self.p
        with np.errstate(all="ignore"):
            z = (self.planes[self.cols] - self.zs[:p, None, :, 0]) * self.zs[:p, None, :, 1]
        out = np.concatenate([z, self.planes[self.ycol][None]])
        for k in range(p + 1):
            poison_cells(out[k], ~self.rows, phase=k + 1)
        return out

    def _group(self, t, rb, raw):
        """(G, M, n) of date t, row-block rb: longdouble (real) or int64 4 G (int; M None)."""
        key = (t, rb, raw)
        g = self._groups.get(key)
        if g is None:
            aa = np.flatnonzero(self.rows[t, rb * 64:(rb + 1) * 64]) + rb * 64
            D = self.design(np.full(len(aa), t), aa, raw)
            g = (gram_int4(D), None, len(aa)) if self.kind == "int" else gram_exact(D)
            self._groups[key] = g
        return g

    def ref(self, t0, t1, a0, a1, raw=False):
        """The Gram over the rows of dates [t0, t1), assets [a0, a1) (multiples of 64; the row set
        ends at A_END by itself) -> (G, M, n).  real: G, M longdouble.  int: G the exact fp64 Gram,
        M None."""
        assert a0 % 64 == 0 and a1 % 64 == 0
        K = self.p + 2
        exact = self.kind == "int"
        G = np.zeros((K, K), np.int64 if exact else LD)
        M = None if exact else np.zeros((K, K), LD)
        n = 0
        for t in range(t0, t1):
            for rb in range(a0 // 64, min(a1, LDA) // 64):
                g, m, k = self._group(t, rb, raw)
                G, n = G + g, n + k
                if not exact:
                    M = M + m
        if exact:
            assert np.abs(G).max(initial=0) < 2 ** 53
            G = G.astype(np.float64) / 4.0
        return G, M, n


_PANELS = {}


def make_panel(p, kind="real", seed=11):
    """The shared panel of (p, kind); built once, never modified by its users."""
    key = (p, kind, seed)
    if key not in _PANELS:
        _PANELS[key] = Panel(p, kind, seed)
    return _PANELS[key]


def scattered_stats(pn, seed=5):
    """The panel's statistics behind a ``zcols`` indirection -> (zs [p+5][LDA][2], zcols [p], zid):
    feature j's row is zs[zcols[j]] (a random injection), the identity row is zs[zid] (a row in
    the middle), the four unused rows are NaN."""
    p = pn.p
    rng = np.random.default_rng([seed, p])
    zid = (p + 5) // 2
    free = np.delete(np.arange(p + 5), zid)
    zcols = rng.permutation(free)[:p].astype(np.int32)
    zs = np.full((p + 5, LDA, 2), np.nan)
    zs[zcols] = pn.zs[:p]
    zs[zid] = pn.zs[p]
    return zs, zcols, zid


# ---- afm_zpredict_f64 ----------------------------------------------------------------------------
def zpredict_seq(beta, x, mu, rs):
    """beta [p+1], x [p][...], mu, rs [p][...] (broadcastable) -> s = beta[0], then for ascending j
    with beta[1+j] != 0: s = s + beta[1+j] * ((x_j - mu_j) * rs_j), every operation rounded to
    fp64 on its own (the kernel's order; zero coefficients of either sign are skipped)."""
    shape = np.broadcast_shapes(*(np.shape(a)[1:] for a in (x, mu, rs)))
    s = np.full(shape, beta[0], dtype=np.float64)
    for j in range(len(beta) - 1):
        if beta[1 + j] != 0.0:
            s = s + beta[1 + j] * ((x[j] - mu[j]) * rs[j])
    return s
