"""Every kernel of csrc/risk.hip against tests/risk_ref.py, bit for bit: the residuals, the factor
covariance, the specific variance and its fill on panels that cross a 64-date bit word and a
64-security block (with NaN-poisoned pad columns, securities never present, listed late and
stopping, a date with too few rows and one with a dropped regressor), the min_obs and lag
boundaries, the books' covariance and risk rows for every solver size with filled members and
dates without a forecast, run-to-run identity and the argument checks."""
import functools

import numpy as np
import pytest

import risk_ref as R
from helpers import same

pytestmark = pytest.mark.gpu

TS, AS, PS = (1, 40, 70), (1, 63, 64, 70, 129), (1, 3, 31)


@functools.lru_cache(maxsize=None)
def panel(T, A, p, seed=0):
    """-> dict: host planes X [p][T][A], y, mask [T][A], and the device base [p+1][T][lda] / bits."""
    import torch
    from afm.grid import pack_bits
    rng = np.random.default_rng([T, A, p, seed])
    lda = (A + 63) // 64 * 64
    X = rng.standard_normal((p, T, A))
    b = rng.normal(0, 0.01, p + 1)
    y = b[0] + np.tensordot(b[1:], X, axes=1) + rng.normal(0, 0.02, (T, A)) * \
        rng.uniform(0.5, 2.0, A)
    mask = rng.random((T, A)) < 0.9
    if A > 3:
        mask[:, 0] = False                            # never present
        mask[:T // 2, 1] = False                      # listed late
        mask[2 * T // 3:, 2] = False                  # stops
    if T > 5:
        mask[3, p:] = False                           # fewer rows than p + 1
        X[0, 5, :] = 1.5                              # a constant column: the regressor is dropped
    X[rng.random(X.shape) < 0.01] = np.nan
    y[rng.random(y.shape) < 0.01] = np.inf
    base = np.full((p + 1, T, lda), np.nan)           # pad columns poisoned
    base[:p, :, :A], base[p, :, :A] = X, y
    m = np.zeros((T, lda), dtype=bool)
    m[:, :A] = mask
    m[:, A:] = True                                   # a set bit on a pad column must not count
    dev = torch.device("cuda", torch.cuda.current_device())
    return dict(T=T, A=A, p=p, lda=lda, X=X, y=y, mask=mask,
                base=torch.from_numpy(base).to(dev), bits=pack_bits(torch.from_numpy(m).to(dev)))


def fit(c, prm):
    from afm.risk import fit_device
    return fit_device(c["base"], list(range(c["p"])), c["p"], c["bits"], prm, T=c["T"], A=c["A"],
                      lda=c["lda"])


def host(res, *keys):
    return [res[k].cpu().numpy() for k in keys]


def check_model(c, res, prm):
    A = c["A"]
    beta, rank, resid, fcov, nused, spec, fill = host(res, "beta", "rank", "resid", "fcov", "nused",
                                                      "spec", "fill")
    u = R.residuals(c["X"], c["y"], c["mask"], beta, rank)
    assert same(resid[:, :A], u) and np.isnan(resid[:, A:]).all()
    f, n = R.factor_cov(beta, rank, prm.half_life, prm.min_obs, prm.lag)
    assert same(nused, n) and same(fcov, f)
    s, fl = R.specific(u, prm.spec_hl, prm.min_obs, prm.lag)
    assert same(spec[:, :A], s) and np.isnan(spec[:, A:]).all()
    assert same(fill, fl)
    return beta, rank, u


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("T", TS)
def test_model_kernels_equal_the_statement(T, A, p):
    from afm.risk import RiskParams
    c = panel(T, A, p)
    i = TS.index(T) + AS.index(A) + PS.index(p)
    prm = RiskParams(half_life=(7.0, 30.0)[i % 2], spec_half_life=(None, 11.0)[(i // 2) % 2],
                     min_obs=(1, 3, 6)[i % 3], lag=(1, 0, 3)[(i // 3) % 3])
    res = fit(c, prm)
    beta, rank, u = check_model(c, res, prm)
    used = R.used_dates(beta, rank)
    if T > 5 and A >= 2 * p + 8:                      # the special dates are what they claim to be
        assert np.isnan(beta[3]).all() and rank[5] == p - 1 and not used[3] and not used[5]
        assert used.any() and np.isfinite(u).any()
    if A <= p:                                        # never enough rows: nothing is used
        assert not used.any()
        assert np.isnan(res["fcov"].cpu().numpy()).all()


def test_min_obs_and_lag_boundaries():
    from afm.risk import RiskParams, model_device
    c = panel(40, 70, 3)
    res = fit(c, RiskParams(min_obs=1, lag=0))
    beta, rank = res["beta"], res["rank"]
    cnt = int(R.used_dates(*host(res, "beta", "rank")).sum())
    assert 30 <= cnt < 40
    for lag in (0, 1, 3):
        for min_obs in (cnt - 1, cnt, cnt + 1):
            prm = RiskParams(half_life=12.0, min_obs=min_obs, lag=lag)
            out = model_device(c["base"], list(range(3)), 3, c["bits"], beta, rank, prm, T=40,
                               A=70, lda=c["lda"])
            check_model(c, out, prm)
            finite = np.isfinite(out["fcov"].cpu().numpy()).all(axis=(1, 2))
            if min_obs > cnt:                         # one more than the panel ever has
                assert not finite.any()
            elif lag == 0:                            # reached on the last used date at the latest
                assert finite[-1] and not finite[:min_obs - 1].any()
    # a lag past the panel: nothing is ever due
    prm = RiskParams(min_obs=1, lag=40)
    out = model_device(c["base"], list(range(3)), 3, c["bits"], beta, rank, prm, T=40, A=70,
                       lda=c["lda"])
    check_model(c, out, prm)
    assert np.isnan(out["fcov"].cpu().numpy()).all() and not out["nused"].any()


def make_books(c, res, k, nd_dates, seed, overlap=True):
    """Random books of k names per side at the given dates (one date with a smaller book, one
    empty), the never-present security 0 among them, the two sides sharing names."""
    import torch
    rng = np.random.default_rng([k, seed])
    nd, A = len(nd_dates), c["A"]
    ks = np.full(nd, k, dtype=np.int32)
    if nd > 2:
        ks[1], ks[2] = max(k // 2, 1), 0
    ids = np.full((nd, 2, 128), -1, dtype=np.int32)
    w = np.zeros((nd, 2, 128))
    for i in range(nd):
        n = int(ks[i])
        if n == 0:
            continue
        L = rng.choice(A, size=n, replace=False)
        if 0 not in L:
            L[rng.integers(n)] = 0                    # spec is NaN there: filled
        rest = np.setdiff1d(np.arange(A), L)
        S = rng.choice(rest, size=n, replace=False)
        if overlap:
            S[: (n + 1) // 2] = rng.permutation(L)[: (n + 1) // 2]   # names on both sides
            S = rng.permutation(S)
        ids[i, 0, :n], ids[i, 1, :n] = L, S
        w[i, 0, :n], w[i, 1, :n] = rng.dirichlet(np.ones(n)), rng.dirichlet(np.ones(n))
    dev = c["base"].device
    reb = {"k": torch.from_numpy(ks).to(dev), "books": torch.from_numpy(ids).to(dev),
           "weights": torch.from_numpy(w).to(dev)}
    return reb, ks, ids, w


@pytest.mark.parametrize("p", (3, 31))
@pytest.mark.parametrize("k", (1, 2, 10, 32, 33, 128))
def test_book_kernel_equals_the_statement(k, p):
    import torch
    from afm.risk import RiskParams, book_risk_device
    c = panel(40, 300, p, seed=1)
    res = fit(c, RiskParams(half_life=10.0, min_obs=8, lag=1))
    fcov, spec, fill = host(res, "fcov", "spec", "fill")
    assert np.isnan(spec[:, 0]).all() and np.isnan(fcov[5]).all() and np.isfinite(fcov[39]).all()
    dates = np.array([39, 38, 30, 5, 25, 20], dtype=np.int32)     # date 5: no forecast yet
    fill2 = fill.copy()
    fill2[25] = np.nan                                # a fill that is needed and missing
    model = dict(res, fill=torch.from_numpy(fill2).to(c["base"].device))
    reb, ks, ids, w = make_books(c, res, k, dates, seed=p)
    dt = torch.from_numpy(dates).to(c["base"].device)
    for kc in sorted({k, min(128, k + 3)}):
        out = book_risk_device(model, c["base"], reb, dt, T=40, lda=c["lda"], kc=kc)
        cov, risk, contrib, status = host(out, "cov", "risk", "contrib", "status")
        rc, rr, rcon, rs = R.books(c["X"], dates, ks, ids, w, fcov, spec, fill2, kc)
        assert status.tolist() == rs.tolist() == [0, 0, 0, 4, 4, 0]
        assert same(cov, rc) and same(risk, rr) and same(contrib, rcon)
        assert risk[0, 0, 3] >= 1 and np.isfinite(risk[[0, 1, 5]]).all()
        assert same(cov[0, 0, :k, :k], cov[0, 0, :k, :k].T)
        again = book_risk_device(model, c["base"], reb, dt, T=40, lda=c["lda"], kc=kc)
        for key in ("cov", "risk", "contrib", "status"):
            assert again[key].cpu().numpy().tobytes() == out[key].cpu().numpy().tobytes(), key


def test_books_without_shared_names_and_a_book_over_kc():
    import torch
    from afm.risk import RiskParams, book_risk_device
    c = panel(40, 300, 3, seed=1)
    res = fit(c, RiskParams(half_life=10.0, min_obs=8, lag=0))
    fcov, spec, fill = host(res, "fcov", "spec", "fill")
    dates = np.array([39, 12, 20], dtype=np.int32)
    reb, ks, ids, w = make_books(c, res, 128, dates, seed=9, overlap=False)   # a union of 256
    dt = torch.from_numpy(dates).to(c["base"].device)
    out = book_risk_device(res, c["base"], reb, dt, T=40, lda=c["lda"], kc=128)
    rc, rr, rcon, rs = R.books(c["X"], dates, ks, ids, w, fcov, spec, fill, 128)
    assert same(out["risk"].cpu().numpy(), rr) and same(out["contrib"].cpu().numpy(), rcon)
    assert same(out["cov"].cpu().numpy(), rc) and out["status"].tolist() == rs.tolist()
    small = book_risk_device(res, c["base"], reb, dt, T=40, lda=c["lda"], kc=64)
    assert small["status"].tolist() == [2, 0, 0]      # date 1 holds 64 names, date 2 none
    assert np.isnan(small["risk"][0].cpu().numpy()).all()
    assert same(small["risk"][1].cpu().numpy(), rr[1])


def test_model_is_identical_run_to_run():
    from afm.risk import RiskParams
    c = panel(70, 129, 31)
    prm = RiskParams(half_life=20.0, min_obs=4, lag=1)
    a, b = fit(c, prm), fit(c, prm)
    for key in ("resid", "fcov", "nused", "spec", "fill"):
        assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), key


def test_fill_sums_more_than_one_run_of_8192():
    """The fill of a date with more than 8192 finite values: numpy's buffered reduction."""
    import torch
    from afm import _lib
    rng = np.random.default_rng(5)
    T, A = 3, 20000
    lda = (A + 63) // 64 * 64
    u = rng.normal(0, 0.02, (T, A))
    u[rng.random((T, A)) < 0.1] = np.nan
    u[1, :9000] = np.nan                              # date 1 (lag 0) leaves under 8192 + a run
    ud = np.full((T, lda), np.nan)
    ud[:, :A] = u
    dev = torch.device("cuda", torch.cuda.current_device())
    resid = torch.from_numpy(ud).to(dev)
    spec = torch.empty((T, lda), dtype=torch.float64, device=dev)
    fill = torch.empty(T, dtype=torch.float64, device=dev)
    _lib.run("afm_risk_specific_f64", resid, T, A, lda, 5.0, 1, 0, spec, fill)
    s, fl = R.specific(u, 5.0, 1, 0)
    assert np.isfinite(s[2]).sum() > 2 * 8192
    assert same(spec.cpu().numpy()[:, :A], s) and same(fill.cpu().numpy(), fl)


def test_bad_arguments_are_rejected():
    import torch
    from afm import _lib
    from afm._lib import AfmError
    c = panel(40, 70, 3)
    dev = c["base"].device
    T, A, lda = 40, 70, c["lda"]
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    beta, rank = torch.zeros((T, 33), **f64), torch.zeros(T, **i32)
    fcov, nused = torch.empty((T, 33, 33), **f64), torch.empty(T, **i32)
    plane, fill = torch.empty((T, lda), **f64), torch.empty(T, **f64)
    cols = torch.arange(32, **i32)
    for p, hl, mo, lag, word in ((32, 9.0, 1, 0, "AFM_RISK_MAX_FACTORS"), (0, 9.0, 1, 0, "p"),
                                 (3, 0.0, 1, 0, "half_life"), (3, -1.0, 1, 0, "half_life"),
                                 (3, float("nan"), 1, 0, "half_life"), (3, 9.0, 0, 0, "min_obs"),
                                 (3, 9.0, 1, -1, "lag")):
        with pytest.raises(AfmError, match=word):
            _lib.run("afm_risk_factor_cov_f64", beta, rank, T, p, hl, mo, lag, fcov, nused)
    for hl, mo, lag in ((0.0, 1, 0), (9.0, 0, 0), (9.0, 1, -1)):
        with pytest.raises(AfmError, match="afm_risk_specific_f64"):
            _lib.run("afm_risk_specific_f64", plane, T, A, lda, hl, mo, lag, plane.clone(), fill)
    with pytest.raises(AfmError, match="shape"):
        _lib.run("afm_risk_specific_f64", plane, T, A, 100, 9.0, 1, 0, plane.clone(), fill)
    with pytest.raises(AfmError, match="AFM_RISK_MAX_FACTORS"):
        _lib.run("afm_risk_resid_f64", c["base"], T * lda, T, A, lda, cols, 32, 3, beta, rank,
                 c["bits"], plane)
    k = torch.zeros(1, **i32)
    books, w = torch.zeros((1, 2, 128), **i32), torch.zeros((1, 2, 128), **f64)
    for kc in (0, 129):
        with pytest.raises(AfmError, match="kc"):
            _lib.run("afm_risk_book_f64", c["base"], T * lda, T, lda, cols, 3, k, 1, k, books, w,
                     fcov, plane, fill, kc, torch.empty((1, 2, 128, 128), **f64),
                     torch.empty((1, 3, 4), **f64), torch.empty((1, 3, 4), **f64), k.clone())
