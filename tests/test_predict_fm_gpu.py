"""afm_predict_f64, afm_fama_macbeth_f64 and the refinement helpers (afm_ols_residual_f64,
afm_vec_add_f64, afm_ols_intercept_f64) called directly at their edges, against the sequential
fp64 restatements and longdouble references of tests/ols_ref.py.

The library is built without FMA contraction and the kernels document their operation order, so
predictions, residuals and the intercept are compared bit for bit; the Fama-MacBeth statistics use
the project's tolerances of test_cross_sectional_ols_vs_oracle (mean 1e-10, t 1e-9)."""
import numpy as np
import pytest

import ols_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FF8DEAD0000BEEF            # a NaN payload no kernel writes
T_PRED = 70                          # crosses a 64-day word
RANGES = [(0, 70), (3, 5), (62, 4), (63, 1), (66, 4)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _handle():
    from afm import _lib
    return _lib.lib(), _lib.ptr, _lib.Context.get(0).bind_stream(), _lib.check


# ---- afm_predict_f64 ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["shared", "per_date", "padded"])
@pytest.mark.parametrize("p", [0, 1, 15, 16, 17, 33, 110])
@pytest.mark.parametrize("lda", [64, 192])
def test_predict(lda, p, mode):
    import torch
    L, P, h, chk = _handle()
    T, K = T_PRED, p + 3
    rng = np.random.default_rng([31, lda, p])
    planes = rng.normal(size=(K, T, lda)) * rng.uniform(0.1, 10.0, size=(K, 1, 1))
    cols = rng.permutation(K - 1)[:p].astype(np.int32)           # plane K-1 is the ycheck plane
    if p >= 2:
        cols[-1] = cols[0]                                       # one plane used twice
    valid = rng.random((T, lda)) < 0.7
    words = R.pack_words(valid)
    words[1] |= rng.integers(0, 2 ** 64, size=lda, dtype=np.uint64) << np.uint64(T - 64)
    if p:                                                        # non-finite regressors, bit set
        tt, aa = np.nonzero(valid)
        pick = rng.choice(len(tt), size=9, replace=False)
        for i, k in enumerate(pick):
            planes[cols[rng.integers(0, p)], tt[k], aa[k]] = (np.nan, np.inf, -np.inf)[i % 3]
    yc = planes[K - 1]
    yc[rng.random((T, lda)) < 0.1] = np.nan
    yc[rng.random((T, lda)) < 0.03] = np.inf
    yc[rng.random((T, lda)) < 0.03] = -np.inf
    stride = {"shared": 0, "per_date": p + 1, "padded": p + 4}[mode]
    if stride == 0:
        beta = rng.normal(size=p + 1)
        bref = beta
    else:
        beta = np.full((T, stride), 1e300)                       # padding must never be read
        beta[:, :p + 1] = rng.normal(size=(T, p + 1))
        bref = beta[:, None, :p + 1]
    x = planes[cols] if p else np.zeros((0, T, lda))
    seq = R.predict_seq(bref, x)
    ld, mag = R.predict_ld(bref, x)
    fin = np.isfinite(seq)
    # the sequential reference itself: within p roundings of the longdouble dot product
    assert float((np.abs(seq[fin] - ld[fin]) / mag[fin]).max()) < 1e-13

    d_planes, d_bits, d_beta = _cuda(planes), _cuda(words.view(np.int64)), _cuda(beta)
    d_cols = _cuda(cols if p else np.zeros(1, dtype=np.int32))
    for ycheck in (-1, K - 1):
        use = valid & (np.isfinite(yc) if ycheck >= 0 else True)
        for t0, nt in RANGES:
            pred = torch.full((T, lda), SENT, dtype=torch.int64, device="cuda").view(torch.float64)
            b = d_beta if stride == 0 else d_beta[t0:]
            chk(L.afm_predict_f64(h, P(d_planes), T * lda, lda, t0, nt, P(d_cols), p, P(b),
                                  stride, P(d_bits), ycheck, P(pred)), "afm_predict_f64")
            torch.cuda.synchronize()
            got = pred.cpu().numpy()
            what = (lda, p, mode, ycheck, t0, nt)
            inside = np.zeros((T, lda), dtype=bool)
            inside[t0:t0 + nt] = True
            assert (_bits(got)[~inside] == np.int64(SENT)).all(), what
            off = inside & ~use
            assert np.isnan(got[off]).all() and (_bits(got)[off] != np.int64(SENT)).all(), what
            on = inside & use
            num = on & ~np.isnan(seq)
            assert (_bits(got)[num] == _bits(seq)[num]).all(), what
            assert np.isnan(got[on & np.isnan(seq)]).all(), what
            okf = on & fin
            assert float((np.abs(got[okf] - ld[okf]) / mag[okf]).max(initial=0.0)) < 1e-13, what


# ---- afm_fama_macbeth_f64 -----------------------------------------------------------------------
def _fm(beta, rank, nseg):
    import torch
    L, P, h, chk = _handle()
    k = beta.shape[1]
    d_beta = _cuda(beta if len(beta) else np.zeros((1, k)))      # nseg = 0: still a buffer
    d_rank = _cuda(np.asarray(rank if len(rank) else [0], dtype=np.int32))
    m = torch.full((k,), 7.0, dtype=torch.float64, device="cuda")
    t = torch.full((k,), 7.0, dtype=torch.float64, device="cuda")
    chk(L.afm_fama_macbeth_f64(h, P(d_beta), P(d_rank), nseg, k, P(m), P(t)), "fama_macbeth")
    torch.cuda.synchronize()
    return m.cpu().numpy(), t.cpu().numpy()


@pytest.mark.parametrize("nseg", [0, 1, 2, 255, 256, 257, 1000])
@pytest.mark.parametrize("k", [1, 31, 111])
def test_fama_macbeth(k, nseg):
    """Rows with rank 0 hold NaN (what the solver writes) and must not reach the result; the
    offset of 1e3 against a unit spread stresses the two-pass variance."""
    rng = np.random.default_rng([37, k, nseg])
    beta = 1e3 + rng.normal(size=(nseg, k))
    rank = np.where(rng.random(nseg) < 0.1, 0, rng.integers(1, 5, size=nseg)).astype(np.int32)
    beta[rank == 0] = np.nan
    m, t = _fm(beta, rank, nseg)
    mref, tref = R.fm_ref(beta, rank)
    used = int((rank > 0).sum())
    assert np.allclose(m, mref, rtol=1e-10, atol=0, equal_nan=True), (used, m[:3], mref[:3])
    assert np.allclose(t, tref, rtol=1e-9, atol=0, equal_nan=True), (used, t[:3], tref[:3])
    assert np.isnan(mref).all() == (used == 0) and np.isnan(tref).all() == (used < 2)


def test_fama_macbeth_degenerate_segment_sets():
    rng = np.random.default_rng(41)
    k, nseg = 5, 300
    beta = 1e3 + rng.normal(size=(nseg, k))
    nanrows = np.full((nseg, k), np.nan)
    # no usable row
    m, t = _fm(nanrows, np.zeros(nseg, dtype=np.int32), nseg)
    assert np.isnan(m).all() and np.isnan(t).all()
    m, t = _fm(np.zeros((0, k)), np.zeros(0, dtype=np.int32), 0)
    assert np.isnan(m).all() and np.isnan(t).all()
    # exactly one usable row, past the first 256-thread stride
    rank = np.zeros(nseg, dtype=np.int32)
    rank[257] = 3
    one = nanrows.copy()
    one[257] = beta[257]
    m, t = _fm(one, rank, nseg)
    assert (m == beta[257]).all() and np.isnan(t).all()
    # identical usable rows: zero spread, t = +-inf with the sign of the mean (as pandas' mean /
    # (std / sqrt(n)) gives).  Quarter-integer values keep every partial sum exact, so the mean is
    # the common value itself and the squared deviations are exactly zero.
    row = np.array([1.25, -2.5, 1024.75, -0.25, 3.0])
    rank = np.where(rng.random(nseg) < 0.1, 0, 2).astype(np.int32)
    same = np.where((rank > 0)[:, None], row, np.nan)
    m, t = _fm(same, rank, nseg)
    assert (m == row).all()
    assert (t == np.where(row > 0, np.inf, -np.inf)).all()
    mref, tref = R.fm_ref(same, rank)
    assert (mref == m).all() and (tref == t).all()


# ---- refinement helpers -------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 17, 110])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_residual_vec_add_intercept(n, p):
    """r is written into a column of Z itself (as LinearRegression.fit does) that is followed by
    the y column and one more: elements past n -- the next columns -- must stay untouched."""
    import torch
    L, P, h, chk = _handle()
    rng = np.random.default_rng([43, n, p])
    Z = rng.normal(size=(p + 3, n)) * 3.0 + 1.0
    rcol, ycol = p, p + 1
    mean = rng.normal(size=p + 2) + 1.0
    beta = rng.normal(size=p + 1)
    d_Z, d_mean, d_beta = _cuda(Z), _cuda(mean), _cuda(beta)
    chk(L.afm_ols_residual_f64(h, P(d_Z), n, p, ycol, P(d_mean), P(d_beta), P(d_Z[rcol])),
        "ols_residual")
    torch.cuda.synchronize()
    got = d_Z.cpu().numpy()
    ref = Z.copy()
    ref[rcol] = R.residual_seq(Z, p, ycol, mean, beta)
    assert (_bits(got) == _bits(ref)).all()

    pad = 5
    x = rng.normal(size=n)
    yv = np.concatenate([rng.normal(size=n), np.zeros(pad)])
    _bits(yv)[n:] = np.int64(SENT)
    d_y = _cuda(yv)
    chk(L.afm_vec_add_f64(h, n, P(_cuda(x)), P(d_y)), "vec_add")
    torch.cuda.synchronize()
    want = yv.copy()
    want[:n] = yv[:n] + x
    assert (_bits(d_y.cpu().numpy()) == _bits(want)).all()

    chk(L.afm_ols_intercept_f64(h, p, P(d_mean), P(d_beta)), "ols_intercept")
    torch.cuda.synchronize()
    want = beta.copy()
    want[0] = R.intercept_seq(p, mean, beta)
    assert (_bits(d_beta.cpu().numpy()) == _bits(want)).all()
