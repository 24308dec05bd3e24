"""The boosted-tree kernels of csrc/gbt.hip called directly, bit for bit against tests/gbt_ref.py:
values and bins, one level's histograms under every work split, one round at its edges, 25 rounds,
and the per-round moments (the only floating-point sums: bitwise repeatable, within the standard
bound of math.fsum)."""
import math

import numpy as np
import pytest

import gbt_ref as R

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dense(X):
    """host [n][p] -> device planes [p][1][n_pad], n_pad."""
    import torch
    n, p = X.shape
    n_pad = (n + 63) // 64 * 64
    base = torch.zeros((p, 1, n_pad), dtype=torch.float64, device="cuda")
    base[:, 0, :n] = _dev(X.T)
    return base, n_pad


# ---- values and bins --------------------------------------------------------------------------
@pytest.mark.parametrize("z", [False, True])
@pytest.mark.parametrize("B", [2, 256])
@pytest.mark.parametrize("p", [1, 97])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_values_and_bins(n, p, B, z):
    """Rows scattered over a [T][lda] panel (row lists), optional z statistics; column 0 is
    constant (no cut) when p > 1, and every cut is itself a value of some row."""
    import torch
    from afm import _lib
    rng = np.random.default_rng(1000 * n + 10 * p + B + z)
    T, lda = 7, 192
    planes = rng.standard_normal((p + 2, T, lda))
    cols = (np.arange(p) + 2).astype(np.int32) if p > 1 else np.array([1], np.int32)
    planes[cols[::3]] = np.round(planes[cols[::3]] * 4) / 4        # ties
    if p > 1:
        planes[cols[0]] = 0.75
    zs = np.stack([rng.standard_normal((p, lda)), 1 / (0.5 + rng.random((p, lda)))], axis=-1)
    cells = rng.choice(T * lda, size=n, replace=n > T * lda)
    rt, ra = (cells // lda).astype(np.int32), (cells % lda).astype(np.int32)
    w = rng.integers(0, 3, size=n).astype(np.int32)
    w[0] = 1
    X = planes[cols][:, rt, ra].T                                  # [n][p]
    if z:
        X = (X - zs[:, ra, 0].T) * zs[:, ra, 1].T
    cuts, ncuts = R.make_cuts(X, w, B)
    want = R.bin_matrix(X, cuts, ncuts)
    if p > 1 and not z:
        assert ncuts[0] == 1 and (want[0, :n] == 1).all()      # a constant column: one cut, itself
    assert any(np.isin(X[:, k], cuts[k, :ncuts[k]]).any() for k in range(p))
    d = dict(base=_dev(planes), cols=_dev(cols), zs=_dev(zs) if z else None, rt=_dev(rt),
             ra=_dev(ra))
    n_pad = want.shape[1]
    vals = torch.empty(n, dtype=torch.float64, device="cuda")
    for k in sorted({0, p // 2, p - 1}):
        _lib.run("afm_gbt_values_f64", d["base"], T * lda, T, lda, d["cols"], k, d["zs"], d["rt"],
                 d["ra"], n, vals)
        assert vals.cpu().numpy().tobytes() == np.ascontiguousarray(X[:, k]).tobytes()
    bins = torch.full((p, n_pad), 255, dtype=torch.uint8, device="cuda")
    _lib.run("afm_gbt_bin_f64", d["base"], T * lda, T, lda, d["cols"], p, d["zs"], d["rt"], d["ra"],
             n, n_pad, _dev(cuts), _dev(ncuts), B, bins)
    assert np.array_equal(bins.cpu().numpy(), want)
    # a column given no cut at all (ncuts = 0): every row in bin 0
    none = ncuts.copy()
    none[0] = 0
    _lib.run("afm_gbt_bin_f64", d["base"], T * lda, T, lda, d["cols"], p, d["zs"], d["rt"], d["ra"],
             n, n_pad, _dev(cuts), _dev(none), B, bins)
    got = bins.cpu().numpy()
    assert (got[0] == 0).all() and np.array_equal(got[1:], want[1:])


def test_constant_column_and_dense_addressing():
    """A dense matrix is T = 1, lda = n_pad, no row lists; a constant training column has one
    candidate (itself): every row is in bin 1, and with a single distinct value below it, 0."""
    import torch
    from afm import _lib
    from afm.gbt import device_cuts
    rng = np.random.default_rng(5)
    n, p, B = 300, 3, 16
    X = rng.standard_normal((n, p))
    X[:, 1] = -2.5
    w = np.ones(n, np.int32)
    w[:40] = 0
    X[:40, 1] = -3.0                                               # only rows that do not train
    cuts, ncuts = R.make_cuts(X, w, B)
    assert ncuts[1] == 1
    base, n_pad = _dense(X)
    cols = torch.arange(p, dtype=torch.int32, device="cuda")
    dc, dn = device_cuts(base, cols, _dev(w), T=1, lda=n_pad, col_stride=n_pad, zs=None,
                         rows_t=None, rows_a=None, n=n, max_bin=B)
    assert dc.cpu().numpy().tobytes() == cuts.tobytes() and np.array_equal(dn.cpu().numpy(), ncuts)
    bins = torch.empty((p, n_pad), dtype=torch.uint8, device="cuda")
    _lib.run("afm_gbt_bin_f64", base, n_pad, 1, n_pad, cols, p, None, None, None, n, n_pad, dc, dn,
             B, bins)
    got = bins.cpu().numpy()
    assert np.array_equal(got, R.bin_matrix(X, cuts, ncuts))
    assert (got[1, :40] == 0).all() and (got[1, 40:n] == 1).all()


# ---- histograms -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hist_case():
    rng = np.random.default_rng(11)
    n, p, B = 70_000, 5, 256
    n_pad = (n + 63) // 64 * 64
    bins = np.zeros((p, n_pad), np.uint8)
    bins[:, :n] = rng.integers(0, B, size=(p, n))
    bins[1, :n] = rng.integers(0, 3, size=n)                       # heavy LDS conflicts
    w = rng.integers(0, 3, size=n).astype(np.int32)
    W = int(w.sum())
    lim = 2 ** 61 // W                                             # q near +-2^61 / W
    sign = np.where(np.arange(n) < n // 2, 1, rng.choice([-1, 1], size=n))
    q = (rng.integers(lim - 1000, lim, size=n) * sign * w).astype(np.int64)
    assert 2 ** 60 < sum(abs(int(v)) for v in q) < 2 ** 62
    return n, n_pad, p, B, bins, q, w


@pytest.mark.parametrize("nnodes", [1, 32])
def test_hist_against_python_sums_under_every_work_split(hist_case, nnodes):
    import torch
    from afm import _lib
    n, n_pad, p, B, bins, q, w = hist_case
    rng = np.random.default_rng(nnodes)
    node = rng.integers(-1, nnodes, size=n).astype(np.int32)
    node[:5] = [-1, nnodes - 1, 0, -1, nnodes - 1]
    want = R.histogram(bins, node, q, w, nnodes, B)
    assert (node == -1).any() and want[..., 1].sum() == p * int(w[node >= 0].sum())
    d = [_dev(a) for a in (bins, node, q, w)]
    got = []
    for rows in (0, 64, 4096):
        hist = torch.full((nnodes, p, B, 2), -7, dtype=torch.int64, device="cuda")
        with _lib.options(gbt_rows_per_wg=rows):
            _lib.run("afm_gbt_hist_i64", d[0], n, n_pad, p, B, d[1], d[2], d[3], nnodes, hist)
        got.append(hist.cpu().numpy())
    assert np.array_equal(got[0], want)
    assert got[1].tobytes() == got[0].tobytes() == got[2].tobytes()


def test_hist_small_shapes_and_bad_arguments():
    import torch
    from afm import _lib
    rng = np.random.default_rng(2)
    for n, p, B, nnodes in ((1, 1, 2, 1), (63, 17, 16, 3), (65, 97, 256, 2), (1001, 2, 5, 32)):
        n_pad = (n + 63) // 64 * 64
        bins = np.zeros((p, n_pad), np.uint8)
        bins[:, :n] = rng.integers(0, B, size=(p, n))
        node = rng.integers(-1, nnodes, size=n).astype(np.int32)
        w = rng.integers(0, 3, size=n).astype(np.int32)
        q = (rng.integers(-2 ** 40, 2 ** 40, size=n) * w).astype(np.int64)
        hist = torch.empty((nnodes, p, B, 2), dtype=torch.int64, device="cuda")
        _lib.run("afm_gbt_hist_i64", _dev(bins), n, n_pad, p, B, _dev(node), _dev(q), _dev(w),
                 nnodes, hist)
        assert np.array_equal(hist.cpu().numpy(), R.histogram(bins, node, q, w, nnodes, B))
    b, nd, qq, ww = _dev(bins), _dev(node), _dev(q), _dev(w)
    good = [b, n, n_pad, p, B, nd, qq, ww, nnodes, hist]
    for i, v in ((1, 0), (1, 1 << 31), (2, n_pad + 1), (2, 64), (3, 0), (3, 257), (4, 1),
                 (4, 257), (8, 0), (8, 33), (0, None), (5, None), (9, None)):
        args = list(good)
        args[i] = v
        with pytest.raises(_lib.AfmError, match="afm_gbt_hist_i64"):
            _lib.run("afm_gbt_hist_i64", *args, device=0)


# ---- the fit ----------------------------------------------------------------------------------
def _fit_gpu(X, y, w, **kw):
    """afm.gbt.fit_device on a dense matrix -> host dict like gbt_ref.fit's."""
    import torch
    from afm.gbt import GBTParams, fit_device
    prm = GBTParams(**kw)
    base, n_pad = _dense(X)
    n, p = X.shape
    res = fit_device(base, np.arange(p, dtype=np.int32), _dev(y), _dev(w.astype(np.int32)), prm,
                     T=1, lda=n_pad, n=n)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same_fit(got, want):
    for k in ("cuts", "ncuts", "bins", "feat", "bin", "thr", "val", "F"):
        assert got[k].dtype == want[k].dtype, k
        assert got[k].tobytes() == want[k].tobytes(), k


def _edge_data(seed, n=500, p=4):
    rng = np.random.default_rng(seed)
    X = np.round(rng.standard_normal((n, p)) * 8) / 8
    y = 0.05 * (X[:, 1] > 0.25) - 0.03 * (X[:, 2] < -0.5) + 0.01 * rng.standard_normal(n)
    w = rng.integers(0, 3, size=n).astype(np.int32)
    return X, y, w


@pytest.mark.parametrize("D", [1, 3, 6])
def test_one_round_every_depth(D):
    X, y, w = _edge_data(D)
    kw = dict(n_rounds=1, max_depth=D, eta=0.3, reg_lambda=0.0, max_bin=32, base_score=0.125)
    want = R.fit(X, y, w, **kw)
    assert (want["feat"][0] >= 0).sum() >= D
    _same_fit(_fit_gpu(X, y, w, **kw), want)


def test_one_round_edges():
    X, y, w = _edge_data(7)
    base = dict(n_rounds=1, max_depth=2, eta=0.5, reg_lambda=0.0, max_bin=16)
    # gamma above every gain: the root stays a leaf
    want = R.fit(X, y, w, **base, gamma=1e9)
    assert want["feat"][0].tolist() == [R.LEAF] + [R.ABSENT] * 6
    _same_fit(_fit_gpu(X, y, w, **base, gamma=1e9), want)
    # a min_child_weight that blocks the unconstrained best split
    free = R.fit(X, y, w, **base)
    k, b = int(free["feat"][0, 0]), int(free["bin"][0, 0])
    HL = int(w[free["bins"][k, :len(y)] <= b].sum())
    mcw = float(min(HL, int(w.sum()) - HL) + 1)
    want = R.fit(X, y, w, **base, min_child_weight=mcw)
    assert (int(want["feat"][0, 0]), int(want["bin"][0, 0])) != (k, b) and want["feat"][0, 0] >= 0
    _same_fit(_fit_gpu(X, y, w, **base, min_child_weight=mcw), want)
    # every row on one side: a column with one cut below every row; min_child_weight = n blocks all
    Xc = X.copy()
    Xc[:, 0] = 1.0
    want = R.fit(Xc[:, :1], y, w, **base)
    assert want["ncuts"][0] == 1 and (want["bins"][0, :len(y)] == 1).all()
    assert want["feat"][0, 0] == R.LEAF                        # the only candidate has HL = 0
    _same_fit(_fit_gpu(Xc[:, :1], y, w, **base), want)
    # tied gains: a duplicated column and a mirrored one -- the lowest column, then the lowest bin
    Xt = np.stack([X[:, 1], X[:, 1], -X[:, 1]], axis=1)
    want = R.fit(Xt, y, w, **base)
    assert want["feat"][0, 0] == 0
    _same_fit(_fit_gpu(Xt, y, w, **base), want)
    # y == F: gmax = 0, e = 0, and the root's value is -0.0
    z = np.zeros(len(y))
    want = R.fit(X, z, w, **base)
    assert want["e"][0] == 0 and want["feat"][0, 0] == R.LEAF
    assert want["val"][0, 0] == 0 and np.signbit(want["val"][0, 0])
    got = _fit_gpu(X, z, w, **base)
    _same_fit(got, want)
    assert np.signbit(got["val"][0, 0]) and not np.signbit(got["F"]).any()


@pytest.fixture(scope="module")
def fit25():
    rng = np.random.default_rng(25)
    n, p = 3000, 8
    X = rng.standard_normal((n, p))
    X[:, 5] = np.round(X[:, 5] * 2) / 2
    y = 0.3 * np.tanh(X[:, 0] * X[:, 1]) + 0.2 * (X[:, 5] > 0) + 0.002 * rng.standard_normal(n)
    w = rng.choice([0, 1, 1, 1, 2], size=n).astype(np.int32)
    kw = dict(n_rounds=25, max_depth=3, eta=0.3, reg_lambda=1.0, gamma=1e-7,
              min_child_weight=5.0, max_bin=64, base_score=0.001)
    return X, y, w, kw, R.fit(X, y, w, **kw), _fit_gpu(X, y, w, **kw)


def test_25_rounds_against_the_reference_and_two_runs_bitwise(fit25):
    from afm import _lib
    X, y, w, kw, want, got = fit25
    assert len(set(want["e"].tolist())) > 1                        # the scale moves with the fit
    assert (want["feat"] >= 0).sum() > 100
    _same_fit(got, want)
    again = _fit_gpu(X, y, w, **kw)
    with _lib.options(gbt_rows_per_wg=64):
        split = _fit_gpu(X, y, w, **kw)
    for other in (again, split):
        for k in got:
            assert other[k].tobytes() == got[k].tobytes(), k       # the moments included


def test_moments_within_the_bound_of_any_summation_order(fit25):
    """Each moment against math.fsum of its terms: |error| <= n * 2^-53 * sum |term|, the
    standard bound for n additions in any order (the products are one rounding each, the same on
    both sides)."""
    X, y, w, kw, want, got = fit25
    F = np.full(len(y), kw["base_score"])
    for r in range(kw["n_rounds"]):
        F = R.predict(X, want["feat"][:r + 1], want["thr"], want["val"], kw["base_score"])
        for g, m in enumerate((w > 0, w == 0)):
            terms = R.moment_terms(F[m], y[m])
            for c, t in enumerate(terms):
                exact = math.fsum(t)
                bound = len(t) * 2.0 ** -53 * math.fsum(np.abs(t))
                assert abs(got["evals"][r, g, c] - exact) <= bound, (r, g, c)
        assert got["evals"][r, 0, 0] == (w > 0).sum() and got["evals"][r, 1, 0] == (w == 0).sum()
    assert F.tobytes() == got["F"].tobytes()
    rmse, ic = R.metrics(got["evals"][-1, 1])
    assert 0 < rmse < 0.1 and ic > 0.5                              # it learns the valid rows too


def test_fit_rejects_bad_arguments():
    import torch
    from afm import _lib
    n, p, D, B = 100, 2, 2, 16
    n_pad = 128
    i32, f64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float64, device="cuda")
    bins = torch.zeros((p, n_pad), dtype=torch.uint8, device="cuda")
    cuts, ncuts = torch.zeros((p, B - 1), **f64), torch.zeros(p, **i32)
    y, w, F = torch.zeros(n, **f64), torch.ones(n, **i32), torch.zeros(n, **f64)
    trees = [torch.zeros((1, 7), **i32), torch.zeros((1, 7), **i32), torch.zeros((1, 7), **f64),
             torch.zeros((1, 7), **f64)]
    ev = torch.zeros((1, 2, 6), **f64)
    scr = torch.zeros(_lib.run("afm_gbt_scratch_bytes", n, p, D, B, device=0) // 8,
                      dtype=torch.int64, device="cuda")
    good = [bins, n, n_pad, p, cuts, ncuts, y, w, 1, D, B, 0.1, 1.0, 0.0, 1.0, *trees, F, ev, scr]
    _lib.run("afm_gbt_fit_f64", *good)
    for i, v in ((1, 0), (3, 0), (3, 257), (8, 0), (9, 0), (9, 7), (10, 1), (10, 257), (12, -1.0),
                 (13, -1.0), (14, 0.5), (2, 100), (0, None), (6, None), (21, None)):
        args = list(good)
        args[i] = v
        with pytest.raises(_lib.AfmError, match="afm_gbt_fit_f64"):
            _lib.run("afm_gbt_fit_f64", *args, device=0)
    torch.cuda.synchronize()
