"""The attribution kernels of csrc/gbt_shap.hip called directly: the cover against the numpy count
at every shape and work split, and the TreeSHAP contributions bit for bit against
gbt_shap_ref.contribs_pinned -- and within the derived bound (gbt_shap_ref's docstring: 2E, E =
(n_trees 2^D + 2D + 19) u S) of the Shapley values by definition -- on hand-built trees, at the
grid's edges, under a cut date range, and on a fitted ensemble."""
import numpy as np
import pytest

import gbt_ref as R
import gbt_shap_ref as S

pytestmark = pytest.mark.gpu

L, A = S.LEAF, S.ABSENT


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- cover ------------------------------------------------------------------------------------
def _random_structure(rng, R_, D, p, B):
    nn = 2 ** (D + 1) - 1
    feat = np.full((R_, nn), A, np.int32)
    sbin = np.full((R_, nn), -1, np.int32)
    feat[:, 0] = L
    for r in range(R_):
        for v in range(2 ** D - 1):
            if feat[r, v] == L and (v == 0 or rng.random() < 0.75):
                feat[r, v], sbin[r, v] = rng.integers(0, p), rng.integers(0, B - 1)
                feat[r, 2 * v + 1] = feat[r, 2 * v + 2] = L
    return feat, sbin


def _cover_gpu(bins, n, p, w, feat, sbin, D, rows=0):
    import torch
    from afm import _lib
    R_ = len(feat)
    out = torch.full(feat.shape, -7, dtype=torch.int64, device="cuda")
    with _lib.options(gbt_rows_per_wg=rows):
        _lib.run("afm_gbt_cover_i64", _dev(bins), n, bins.shape[1], p, _dev(w), _dev(feat),
                 _dev(sbin), D, R_, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("D", [1, 3, 6])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_cover_equals_the_numpy_count(n, D):
    rng = np.random.default_rng(10 * n + D)
    B = 16
    for p in (1, 97):
        for R_ in (1, 25, 70):                                  # 70: more than one slab of trees
            if R_ == 70 and (n != 1000 or p != 97):
                continue
            n_pad = (n + 63) // 64 * 64
            bins = np.zeros((p, n_pad), np.uint8)
            bins[:, :n] = rng.integers(0, B, size=(p, n))
            bins[:, n:] = 255                                   # padding rows are never read
            w = rng.choice([0, 1, 2, 4095], size=n).astype(np.int32)
            feat, sbin = _random_structure(rng, R_, D, p, B)
            want = S.cover(bins, w, feat, sbin)
            assert (want[:, 0] == w.sum()).all() and (want[feat == A] == 0).all()
            got = _cover_gpu(bins, n, p, w, feat, sbin, D)
            assert got.dtype == np.int64 and np.array_equal(got, want), (p, R_)
            if n == 1000:                                       # several chunks of rows
                assert np.array_equal(_cover_gpu(bins, n, p, w, feat, sbin, D, rows=64), want)
                assert np.array_equal(_cover_gpu(bins, n, p, w, feat, sbin, D, rows=257), want)


@pytest.fixture(scope="module")
def fit25():
    """25 rounds of gbt_ref on 500 x 4 rows, the cover of the kernel on the fit's bins and weights."""
    rng = np.random.default_rng(25)
    n, p = 500, 4
    X = np.round(rng.standard_normal((n, p)) * 8) / 8
    y = 0.3 * np.tanh(X[:, 0] * X[:, 1]) + 0.2 * (X[:, 2] > 0) + 0.002 * rng.standard_normal(n)
    w = rng.choice([0, 1, 1, 1, 2], size=n).astype(np.int32)
    kw = dict(n_rounds=25, max_depth=3, eta=0.3, reg_lambda=1.0, min_child_weight=2.0, max_bin=32,
              base_score=0.001)
    fit = R.fit(X, y, w, **kw)
    cov = _cover_gpu(fit["bins"], n, p, w, fit["feat"], fit["bin"], 3)
    return X, w, kw, fit, cov


def test_cover_of_a_fit_is_the_fits_h(fit25):
    X, w, kw, fit, cov = fit25
    feat = fit["feat"]
    assert np.array_equal(cov, S.cover(fit["bins"], w, feat, fit["bin"]))
    assert (cov[:, 0] == w.sum()).all()
    r, v = np.nonzero(feat >= 0)
    assert len(r) > 100 and (cov[r, v] == cov[r, 2 * v + 1] + cov[r, 2 * v + 2]).all()
    assert (cov[feat != A] >= kw["min_child_weight"]).all() and (cov[feat == A] == 0).all()


def test_cover_rejects_bad_arguments():
    import torch
    from afm import _lib
    n, n_pad, p, D, R_ = 100, 128, 3, 2, 4
    bins = torch.zeros((p, n_pad), dtype=torch.uint8, device="cuda")
    w = torch.ones(n, dtype=torch.int32, device="cuda")
    feat = torch.full((R_, 7), -2, dtype=torch.int32, device="cuda")
    feat[:, 0] = -1
    sbin = torch.full((R_, 7), -1, dtype=torch.int32, device="cuda")
    cov = torch.zeros((R_, 7), dtype=torch.int64, device="cuda")
    good = [bins, n, n_pad, p, w, feat, sbin, D, R_, cov]
    _lib.run("afm_gbt_cover_i64", *good)
    assert cov.cpu().numpy().tolist() == [[100, 0, 0, 0, 0, 0, 0]] * R_      # root leaves
    for i, v in ((1, 0), (1, 1 << 31), (2, n_pad + 1), (2, 64), (3, 0), (3, 257), (7, 0), (7, 7),
                 (8, -1), (8, (1 << 20) + 1), (0, None), (4, None), (5, None), (6, None),
                 (9, None)):
        args = list(good)
        args[i] = v
        with pytest.raises(_lib.AfmError, match="afm_gbt_cover_i64"):
            _lib.run("afm_gbt_cover_i64", *args, device=0)
    cov.fill_(-3)
    args = list(good)
    args[8] = 0
    _lib.run("afm_gbt_cover_i64", *args)                       # no tree: nothing is written
    assert (cov.cpu().numpy() == -3).all()


# ---- contributions: scenes and trees ----------------------------------------------------------
def _cover_from_rows(feat, thr, Xc):
    """The covers a sample of rows gives hand-built trees (raw-value routing: left iff x < thr)."""
    R_, nn = feat.shape
    cov = np.zeros((R_, nn), np.int64)
    for r in range(R_):
        v = np.zeros(len(Xc), np.int64)
        np.add.at(cov[r], v, 1)
        while True:
            k = feat[r][v]
            go = k >= 0
            if not go.any():
                break
            idx = np.flatnonzero(go)
            v[idx] = 2 * v[idx] + 1 + (Xc[idx, k[idx]] >= thr[r][v[idx]])
            np.add.at(cov[r], v[idx], 1)
    assert (cov[feat != A] >= 1).all()
    return cov


def _hand_trees(kind, p, rng):
    """(feat, thr, val, cover, D) of one hand-built ensemble on columns < p."""
    Xc = np.round(rng.standard_normal((4096, p)) * 4) / 4
    if kind == "stump":
        D, feat, thr = 1, np.array([[p - 1, L, L]], np.int32), np.array([[0.25, 0, 0]])
    elif kind == "root_leaf":
        D, feat, thr = 2, np.array([[L] + [A] * 6] * 2, np.int32), np.zeros((2, 7))
    elif kind == "full6":                      # level l splits column l: six columns on every path
        D = 6
        feat = np.full((1, 127), L, np.int32)
        thr = np.zeros((1, 127))
        for v in range(63):
            lvl = (v + 1).bit_length() - 1
            feat[0, v] = (lvl * 3) % p if p >= 16 else lvl
            thr[0, v] = rng.choice([-0.25, 0.0, 0.25])
        assert len(set(feat[0, :63].tolist())) == 6
    elif kind == "chain6":                     # one column six times: m = 1 on every path
        D = 6
        feat = np.full((1, 127), A, np.int32)
        thr = np.zeros((1, 127))
        v = 0
        for t in (1.5, 1.0, 0.5, 0.0, -0.5, -1.0):
            feat[0, v], thr[0, v] = p // 2, t
            feat[0, 2 * v + 2] = L
            v = 2 * v + 1
        feat[0, v] = L
    else:
        raise KeyError(kind)
    val = np.where(feat == L, rng.standard_normal(feat.shape) * 0.05, 0.0)
    return feat, thr, val, _cover_from_rows(feat, thr, Xc), D


class Scene:
    """Planes [P][T][lda] of quarter-rounded values, a row mask with a wholly unset date, a fully
    set one and unset padding assets; NaN poison in every unset cell and in the z statistics of
    the padding assets."""

    def __init__(self, rng, p, T, lda, z):
        self.p, self.T, self.lda = p, T, lda
        P = p + 2
        self.cols = ((np.arange(p) * 7 + 3) % p + 2).astype(np.int32) if p > 1 else \
            np.array([1], np.int32)
        self.planes = np.round(rng.standard_normal((P, T, lda)) * 4) / 4
        use = rng.random((T, lda)) < 0.7
        use[:, lda - 5:] = False
        if T > 1:
            use[T - 2] = False
        use[T - 1, :lda - 5] = True
        self.use = use
        self.planes[:, ~use] = np.nan
        self.zs = None
        if z:
            self.zs = np.stack([np.round(rng.standard_normal((p, lda)) * 2) / 2,
                                rng.choice([0.5, 1.0, 2.0], size=(p, lda))], axis=-1)
            self.zs[:, lda - 5:] = np.nan
        words = np.zeros(lda, np.uint64)
        for t in range(T):
            words |= use[t].astype(np.uint64) << np.uint64(t)
        self.bits = words.view(np.int64).reshape(1, lda)
        self.d = None

    def put(self, t, a, k, x):
        """Make feature k of the set cell (t, a) take the (z-scored) value x exactly."""
        assert self.use[t, a]
        if self.zs is not None:
            x = x / self.zs[k, a, 1] + self.zs[k, a, 0]          # exact: halves and powers of two
        self.planes[self.cols[k], t, a] = x

    def X(self, t):
        """(assets, X [n][p]) of the set cells of date t, as the kernels read them."""
        a = np.flatnonzero(self.use[t])
        X = self.planes[self.cols][:, t, a].T
        if self.zs is not None:
            X = (X - self.zs[:, a, 0].T) * self.zs[:, a, 1].T
        return a, X

    def dev(self):
        if self.d is None:
            self.d = dict(base=_dev(self.planes), cols=_dev(self.cols), bits=_dev(self.bits),
                          zs=None if self.zs is None else _dev(self.zs))
        return self.d


def _shap_gpu(sc, trees, t0, nt, n_trees=None, base_score=0.0, contrib=True, agg=True):
    import torch
    from afm import _lib
    feat, thr, val, cov, D = trees
    R_ = len(feat) if n_trees is None else n_trees
    d = sc.dev()
    p, lda, T = sc.p, sc.lda, sc.T
    nbytes = _lib.run("afm_gbt_shap_scratch_bytes", lda, nt, p, D, R_, device=0)
    scr = torch.full(((nbytes + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    c = torch.full((nt, p + 1, lda), 7.5, **f64) if contrib else None
    g = torch.full((nt, p + 1, 2), 7.5, **f64) if agg else None
    m = torch.full((nt,), -7, dtype=torch.int64, device="cuda") if agg else None
    _lib.run("afm_gbt_shap_f64", d["base"], T * lda, lda, t0, nt, d["cols"], p, d["zs"],
             _dev(feat), _dev(thr), _dev(val), _dev(cov), D, R_, base_score, d["bits"], scr, c, g,
             m)
    return tuple(None if x is None else x.cpu().numpy() for x in (c, g, m))


def _predict_gpu(sc, trees, n_trees, base_score):
    import torch
    from afm import _lib
    feat, thr, val, cov, D = trees
    d = sc.dev()
    pred = torch.full((sc.T, sc.lda), 7.5, dtype=torch.float64, device="cuda")
    _lib.run("afm_gbt_predict_f64", d["base"], sc.T * sc.lda, sc.lda, 0, sc.T, d["cols"], sc.p,
             d["zs"], _dev(feat), _dev(thr), _dev(val), D, n_trees, base_score, d["bits"], pred)
    return pred.cpu().numpy()


def _check(sc, trees, t0, nt, n_trees=None, base_score=0.0, worst=None):
    """One call with every output against the pinned statement (bitwise), the definition (2E) and
    the tree walk (efficiency); returns the outputs."""
    feat, thr, val, cov, D = trees
    R_ = len(feat) if n_trees is None else n_trees
    p = sc.p
    got, agg, cnt = _shap_gpu(sc, trees, t0, nt, R_, base_score)
    use = sc.use[t0:t0 + nt]
    assert np.isnan(got[~np.broadcast_to(use[:, None, :], got.shape)]).all()
    E = S.bound(feat, val, base_score, R_)
    pred = _predict_gpu(sc, trees, R_, base_score)
    for i in range(nt):
        a, X = sc.X(t0 + i)
        if len(a) == 0:
            continue
        assert np.isfinite(X).all()
        want = S.contribs_pinned(X, feat, thr, val, cov, base_score, R_)
        cell = np.ascontiguousarray(got[i][:, a].T)
        assert cell.tobytes() == want.tobytes(), (t0 + i, np.abs(cell - want).max())
        exact = S.contribs_by_definition(X, feat, thr, val, cov, base_score, R_)
        err = float(np.abs(cell.astype(np.longdouble) - exact).max())
        print(f"date {t0 + i}: max error {err:.3e} = {err / E if E else 0.0:.4f} E")
        assert err <= 2 * E
        if worst is not None and E:
            worst.append(err / E)
        total = cell.astype(np.longdouble).sum(axis=1)
        assert np.abs(total - pred[t0 + i, a]).max() <= (p + 1) * 2 * E + E
    want_agg, want_cnt = S.agg_pinned(got, use)
    assert agg.tobytes() == want_agg.tobytes() and np.array_equal(cnt, want_cnt)
    return got, agg, cnt


@pytest.mark.parametrize("z", [False, True])
@pytest.mark.parametrize("kind,p", [("stump", 1), ("stump", 97), ("root_leaf", 1), ("full6", 97),
                                    ("full6", 256), ("full6", 6), ("chain6", 97), ("chain6", 1)])
def test_hand_built_trees_against_pinned_and_definition(kind, p, z):
    rng = np.random.default_rng(len(kind) * 1000 + p * 2 + z)
    trees = _hand_trees(kind, p, rng)
    feat, thr, val, cov, D = trees
    sc = Scene(rng, p, 3, 128, z)
    if (feat[0] >= 0).any():                       # a value exactly on a threshold goes right
        k, t = int(feat[0, 0]), float(thr[0, 0])
        a = int(np.flatnonzero(sc.use[0])[0])
        sc.put(0, a, k, t)
        _, X = sc.X(0)
        assert X[0, k] == t
    got, agg, cnt = _check(sc, trees, 0, 3, base_score=0.375)
    if kind == "root_leaf":
        a, _ = sc.X(0)
        assert (got[0][:p, a] == 0).all() and not np.signbit(got[0][:p, a]).any()
        assert (got[0][p, a] == (0.375 + val[0, 0]) + val[1, 0]).all()
    if kind == "stump":                            # on the threshold: the right leaf's side
        a = int(np.flatnonzero(sc.use[0])[0])
        zl, zr = cov[0, 1] / cov[0, 0], cov[0, 2] / cov[0, 0]
        assert got[0][p - 1, a] == (0.0 + val[0, 1] * (0.0 - zl)) + val[0, 2] * (1.0 - zr)
        assert got[0][p, a] == (0.375 + val[0, 1] * zl) + val[0, 2] * zr
        aa, _ = sc.X(0)
        never = got[0][:p - 1][:, aa]
        assert (never == 0).all() and not np.signbit(never).any()


@pytest.fixture(scope="module")
def forest():
    """Random trees with absent subtrees, depth 4, on 97 columns, and a z-scored scene of 8 dates."""
    rng = np.random.default_rng(77)
    feat, thr, val, cov, _ = S.random_trees(rng, 9, 4, 97, ncols=7, leaf_p=0.35)
    assert (feat == A).sum() > 40 and (feat >= 0).sum() > 30
    return Scene(rng, 97, 8, 128, True), (feat, thr, val, cov, 4)


def test_absent_subtrees_prefixes_and_no_tree(forest):
    sc, trees = forest
    worst = []
    _check(sc, trees, 0, 8, base_score=-0.125, worst=worst)
    _check(sc, trees, 0, 2, n_trees=4, base_score=0.5)
    got, agg, cnt = _check(sc, trees, 0, 8, n_trees=0, base_score=0.625)
    use = sc.use
    for i in range(8):
        assert (got[i][:97][:, use[i]] == 0).all() and (got[i][97][use[i]] == 0.625).all()
    assert (agg[6] == 0).all() and cnt[6] == 0 and cnt[7] == 128 - 5       # unset / full date
    print(f"worst observed fraction of E: {max(worst):.4f}")


@pytest.mark.parametrize("lda", [64, 128])
@pytest.mark.parametrize("t0,nt", [(0, 1), (3, 4), (2, 5)])
def test_grid_edges(lda, t0, nt):
    rng = np.random.default_rng(lda + 10 * t0 + nt)
    feat, thr, val, cov, _ = S.random_trees(rng, 5, 3, 11, ncols=5)
    # the range ends on the wholly unset date, except the one-date range (a partly set date)
    sc = Scene(rng, 11, t0 + nt + (1 if nt > 1 else 2), lda, bool(nt & 1))
    _check(sc, (feat, thr, val, cov, 3), t0, nt, base_score=0.25)


def test_cut_ranges_single_outputs_and_two_runs_are_bitwise_equal(forest):
    sc, trees = forest
    full = _shap_gpu(sc, trees, 1, 7, base_score=0.1)
    again = _shap_gpu(sc, trees, 1, 7, base_score=0.1)
    lo, hi = _shap_gpu(sc, trees, 1, 3, base_score=0.1), _shap_gpu(sc, trees, 4, 4, base_score=0.1)
    only_c = _shap_gpu(sc, trees, 1, 7, base_score=0.1, agg=False)
    only_a = _shap_gpu(sc, trees, 1, 7, base_score=0.1, contrib=False)
    for j in range(3):
        assert again[j].tobytes() == full[j].tobytes()
        assert np.concatenate([lo[j], hi[j]]).tobytes() == full[j].tobytes()
    assert only_c[0].tobytes() == full[0].tobytes() and only_c[1] is None and only_c[2] is None
    assert only_a[0] is None and only_a[1].tobytes() == full[1].tobytes()
    assert np.array_equal(only_a[2], full[2])


def test_fitted_ensemble_bit_for_bit(fit25):
    """The 25-round fit's trees with the kernel's own cover, on the fit's rows as a dense matrix
    (one date, lda = n_pad) and on other rows."""
    X, w, kw, fit, cov = fit25
    rng = np.random.default_rng(9)
    trees = (fit["feat"], fit["thr"], fit["val"], cov, 3)
    sc = Scene(rng, 4, 1, 512, False)
    sc.use[:] = False
    sc.use[0, :500] = True
    sc.planes[:] = np.nan
    sc.cols = np.arange(4, dtype=np.int32) + 2
    sc.planes[sc.cols, 0, :500] = X.T
    words = sc.use[0].astype(np.uint64)
    sc.bits = words.view(np.int64).reshape(1, 512)
    worst = []
    got, agg, cnt = _check(sc, trees, 0, 1, base_score=kw["base_score"], worst=worst)
    _check(sc, trees, 0, 1, n_trees=7, base_score=kw["base_score"])
    assert cnt[0] == 500
    # efficiency against the fit's own F on its rows
    E = S.bound(fit["feat"], fit["val"], kw["base_score"])
    total = got[0][:, :500].astype(np.longdouble).sum(axis=0)
    assert np.abs(total - fit["F"]).max() <= 5 * 2 * E + E
    print(f"worst observed fraction of E: {max(worst):.4f}")


def test_shap_rejects_bad_arguments():
    import torch
    from afm import _lib
    rng = np.random.default_rng(1)
    feat, thr, val, cov, _ = S.random_trees(rng, 2, 2, 3, ncols=3)
    sc = Scene(rng, 3, 2, 64, True)
    d = sc.dev()
    f64 = dict(dtype=torch.float64, device="cuda")
    scr = torch.zeros(_lib.run("afm_gbt_shap_scratch_bytes", 64, 2, 3, 2, 2, device=0) // 8 + 2,
                      dtype=torch.int64, device="cuda")
    c, g = torch.zeros((2, 4, 64), **f64), torch.zeros((2, 4, 2), **f64)
    m = torch.zeros(2, dtype=torch.int64, device="cuda")
    good = [d["base"], 2 * 64, 64, 0, 2, d["cols"], 3, d["zs"], _dev(feat), _dev(thr), _dev(val),
            _dev(cov), 2, 2, 0.0, d["bits"], scr, c, g, m]
    _lib.run("afm_gbt_shap_f64", *good)
    bad = [(2, 0), (2, 100), (3, -1), (4, -1), (6, 0), (6, 257), (12, 0), (12, 7), (13, -1),
           (13, (1 << 20) + 1), (0, None), (5, None), (8, None), (9, None), (10, None), (11, None),
           (15, None), (16, None), (16, scr[1:]), (19, None), (18, None)]
    for i, v in bad:
        args = list(good)
        args[i] = v
        with pytest.raises(_lib.AfmError, match="afm_gbt_shap_f64"):
            _lib.run("afm_gbt_shap_f64", *args, device=0)
    args = list(good)
    args[17] = args[18] = args[19] = None                      # no output at all
    with pytest.raises(_lib.AfmError, match="afm_gbt_shap_f64"):
        _lib.run("afm_gbt_shap_f64", *args, device=0)
    args = list(good)
    args[4] = 0                                                # no date: nothing is written
    c.fill_(3.0)
    _lib.run("afm_gbt_shap_f64", *args)
    torch.cuda.synchronize()
    assert (c.cpu().numpy() == 3.0).all()
