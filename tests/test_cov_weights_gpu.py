"""The weight solves from a supplied covariance (afm_cov_weights_f64, afm_rebalance_cov_f64): fed the
covariance the existing solves formed they return those solves' weights, sums and status bit for
bit (the wave solver up to 32 names, the workgroup solver above, with and without the return term,
both trivial-bound branches); on a factor-model covariance they meet tests/mv_ref.py at the bar
tests/test_mv_weights_gpu.py uses for this solver."""
import numpy as np
import pytest

import mv_ref
from helpers import same
from test_mv_rebalance_gpu import WINDOW, panel, planes, run  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

KS = (2, 9, 32, 33, 128)


@pytest.mark.parametrize("k", KS)
def test_cov_weights_repeat_the_one_book_solves(k):
    from afm.portfolio import mean_variance_weights
    from afm.risk import cov_weights
    rng = np.random.default_rng([3, k])
    R = mv_ref.make_book(rng, k, 90 if k <= 32 else 160, True)
    mu = rng.normal(0, 1e-3, k)
    mu[0] = np.nan                                    # counts as 0 in both
    lo, hi = mv_ref.book_bounds(k)
    # the QP, then w = hi (k * hi <= 1) and w = lo (k * lo >= 1)
    for blo, bhi in ((lo, hi), (0.0, 1.0 / k if k in (2, 32, 128) else 0.9 / k), (1.5 / k, 0.9)):
        for gamma in (0.0, 0.2):
            w, cov, st = mean_variance_weights(R, mu, gamma, blo, bhi, status=True)
            w2, st2 = cov_weights(cov, mu, gamma, blo, bhi, status=True)
            assert same(w2, w) and st2 == st == 0, (k, blo, bhi, gamma)
            w3 = cov_weights(cov, None, gamma, blo, bhi)          # no mu: the min-variance solve
            w0, _ = mean_variance_weights(R, mu, 0.0, blo, bhi)
            assert same(w3, w0)
    w, cov = mean_variance_weights(R, mu, 0.2, lo, hi)
    assert not same(w, mean_variance_weights(R, mu, 0.0, lo, hi)[0])   # the term matters here
    if k > 1:
        assert len(np.unique(w)) > 1


def test_non_finite_covariance_and_bad_arguments():
    from afm._lib import AfmError
    from afm.risk import cov_weights
    S = np.eye(12) * 1e-4
    S[3, 1] = np.nan                                  # the lower triangle is what is read
    w, st = cov_weights(S, None, 0.0, 0.0, 0.2, status=True)
    assert st == 1 and np.isnan(w).all()
    S[3, 1], S[1, 3] = 0.0, np.nan                    # the upper triangle is not
    w, st = cov_weights(S, None, 0.0, 0.0, 0.2, status=True)
    assert st == 0 and np.abs(w - 1 / 12).max() < 1e-15
    for gamma in (-0.1, float("nan"), float("inf")):
        with pytest.raises(AfmError, match="gamma"):
            cov_weights(np.eye(3), None, gamma)
    with pytest.raises(AfmError, match="bad arguments"):
        cov_weights(np.eye(3), None, 0.0, 0.5, 0.1)
    with pytest.raises(ValueError):
        cov_weights(np.eye(129))


@pytest.mark.parametrize("k", KS)
def test_factor_model_covariance_vs_reference(k):
    from afm.risk import cov_weights
    rng = np.random.default_rng([5, k])
    K1 = 6
    B = np.c_[np.ones(k), rng.standard_normal((k, K1 - 1))]
    Z = rng.standard_normal((K1, 40)) * rng.uniform(0.002, 0.01, (K1, 1))
    S = B @ (Z @ Z.T / 40) @ B.T + np.diag(rng.uniform(1e-4, 9e-4, k))
    S = np.tril(S) + np.tril(S, -1).T
    mu = rng.normal(0, 1e-3, k)
    lo, hi = mv_ref.book_bounds(k)
    for gamma in (0.0, 0.2):
        wo, _ = mv_ref.box_qp_mv(S, mu, gamma, lo, hi)
        w, st = cov_weights(S, mu, gamma, lo, hi, status=True)
        err = np.abs(w - wo).max()
        res = mv_ref.kkt_residual(S, mu, gamma, w, lo, hi)
        print(f"k={k} gamma={gamma}: |w - ref| {err:.2e} kkt {res:.2e}")
        assert st == 0 and err < 1e-9 and res < 1e-9
        assert abs(w.sum() - 1) < 1e-12 and w.min() >= lo and w.max() <= hi


def window_covs(g, base, top_n):
    """The covariance of every (date, side) of ``base``, rebuilt from the history planes with the
    one-book solve (the same covariance code on the same rows) -> device [nd][2][top_n][top_n]."""
    import torch
    from afm.portfolio import min_variance_weights
    hist = g["hist"].cpu().numpy()
    k, books = base["k"].cpu().numpy(), base["books"].cpu().numpy()
    rd = g["rdates_np"]
    cov = np.full((len(rd), 2, top_n, top_n), np.nan)
    for i, t in enumerate(rd):
        for s in range(2):
            mem = books[i, s, :k[i]]
            R = hist[max(t - WINDOW, 0):t][:, mem]
            cov[i, s, :k[i], :k[i]] = min_variance_weights(R)[1]
    return torch.from_numpy(cov).to(g["pred"].device)


@pytest.mark.parametrize("top_n", [12, 40])
def test_rebalance_cov_repeats_the_rebalance(planes, top_n):  # noqa: F811
    import torch
    from afm.risk import rebalance_cov_device
    g = planes
    base = run(g, top_n)
    assert (base["k"].cpu().numpy() == top_n).all() and not base["status"].any()
    cov = window_covs(g, base, top_n)
    for gamma, ref in ((0.0, base), (0.05, run(g, top_n, risk_tolerance=0.05, mu=g["pred"]))):
        reb = {key: v.clone() for key, v in base.items()}
        reb["weights"].fill_(7.0)
        reb["sums"].fill_(7.0)
        reb["status"].fill_(1)                        # a stale cap flag is this solve's to clear
        flag = torch.zeros_like(reb["status"])
        flag[3] = 4                                   # no usable covariance on date 3
        rebalance_cov_device(reb, cov, g["rdates"], g["close"], g["tmr"], kc=top_n,
                             cov_status=flag, mu=g["pred"] if gamma else None,
                             risk_tolerance=gamma)
        w, sums, st = (reb[key].cpu().numpy() for key in ("weights", "sums", "status"))
        rw, rs = ref["weights"].cpu().numpy(), ref["sums"].cpu().numpy()
        keep = np.arange(len(st)) != 3
        assert same(w[keep][:, :, :top_n], rw[keep][:, :, :top_n]) and same(sums[keep], rs[keep])
        assert (w[3, :, :top_n] == 7.0).all() and (sums[3] == 7.0).all()
        assert st[keep].tolist() == [0] * keep.sum() and st[3] == 1 | 4
        assert (w[:, :, top_n:] == 7.0).all()         # nothing past the books
        for key in ("k", "books", "upos", "usize"):
            assert same(reb[key].cpu().numpy(), base[key].cpu().numpy()), key
    # mu without a risk tolerance, and no cov_status: the min-variance solve on every date
    reb = {key: v.clone() for key, v in base.items()}
    reb["weights"].zero_()
    rebalance_cov_device(reb, cov, g["rdates"], g["close"], g["tmr"], kc=top_n, mu=g["pred"])
    assert same(reb["weights"].cpu().numpy(), base["weights"].cpu().numpy())
    assert same(reb["sums"].cpu().numpy(), base["sums"].cpu().numpy())


def test_rebalance_cov_rejects_bad_arguments(planes):  # noqa: F811
    import torch
    from afm._lib import AfmError
    from afm.risk import rebalance_cov_device
    g = planes
    base = run(g, 12)
    cov = torch.zeros((int(g["rdates"].numel()), 2, 12, 12), dtype=torch.float64,
                      device=g["pred"].device)
    for kc in (0, 129):
        with pytest.raises(AfmError, match="kc"):
            rebalance_cov_device(base, cov, g["rdates"], g["close"], g["tmr"], kc=kc)
    with pytest.raises(AfmError, match="gamma"):
        rebalance_cov_device(base, cov, g["rdates"], g["close"], g["tmr"], kc=12,
                             risk_tolerance=-1.0)
    # a stride below the books: the dates are left alone
    small = torch.zeros((int(g["rdates"].numel()), 2, 8, 8), dtype=torch.float64,
                        device=g["pred"].device)
    before = base["weights"].clone()
    rebalance_cov_device(base, small, g["rdates"], g["close"], g["tmr"], kc=8)
    assert same(base["weights"].cpu().numpy(), before.cpu().numpy())
