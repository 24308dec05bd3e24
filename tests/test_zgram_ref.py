"""CPU checks of tests/zgram_ref.py: the reference Gram, its derived bound, the exact-integer panel
and the poisoning the GPU tests of the Gram and z-predict kernels rely on."""
import numpy as np
import pytest

import zgram_ref as R

P_GRID = [1, 14, 15, 30, 31, 94, 95, 96, 106]


def _rows(pn, n):
    """the first n rows (date-major) of the panel's row set"""
    tt, aa = np.nonzero(pn.rows)
    assert len(tt) >= n
    return tt[:n], aa[:n]


@pytest.mark.parametrize("p", P_GRID)
def test_numpy_gram_is_well_inside_the_bound(p):
    """numpy's fp64 D D^T against the longdouble Gram at n = 450: below 9 * 2^-53 * M entry by
    entry, so the reference and a correct fp64 summation sit far inside bound(n, M) = 2 n u M."""
    pn = R.make_panel(p, "real")
    D = pn.design(*_rows(pn, 450))
    assert D.shape == (p + 2, 450) and np.isfinite(D).all()
    G, M, n = R.gram_exact(D)
    assert n == 450 and G.dtype == R.LD and np.finfo(R.LD).nmant >= 63
    err = np.abs(R.gram_f64(D).astype(R.LD) - G)
    assert (err <= 9 * R.LD(R.U) * M).all(), float((err / M).max() / R.U)
    assert (err <= R.bound(n, M)).all()
    assert G[0, 0] == 450 and np.array_equal(G, G.T)


@pytest.mark.parametrize("p", P_GRID)
def test_int_panel_is_exact(p):
    """On the integer panel fp64, longdouble and int64 arithmetic give the same Gram, bit for bit
    (with and without the statistics)."""
    pn = R.make_panel(p, "int")
    for raw in (False, True):
        D = pn.design(*_rows(pn, 450), raw=raw)
        G4 = R.gram_int4(D)
        G, _, _ = R.gram_exact(D)
        exp = G4.astype(np.float64) / 4.0
        assert np.array_equal(exp * 4.0, G4)
        assert np.array_equal(R.gram_f64(D).view(np.int64), exp.view(np.int64))
        assert np.array_equal(G, exp.astype(R.LD))
    z = pn.design(*_rows(pn, 450))[1:-1]
    assert np.abs(z).max() <= 20 and len(np.unique(z)) > 30      # not a degenerate draw


@pytest.mark.parametrize("kind", ["real", "int"])
def test_a_dropped_or_doubled_row_breaks_the_bound(kind):
    pn = R.make_panel(30, kind)
    D = pn.design(*_rows(pn, 450))
    G, M, n = R.gram_exact(D)
    for wrong in (D[:, 1:], np.concatenate([D, D[:, :1]], axis=1)):
        err = np.abs(R.gram_f64(wrong).astype(R.LD) - G)
        over = err > R.bound(n, M)
        assert over[0, 0] and over[-1, -1] and over.mean() > 0.8   # (an integer product can be 0)


@pytest.mark.parametrize("kind", ["real", "int"])
def test_panel_is_poisoned_outside_the_row_set(kind):
    p = 15
    pn = R.make_panel(p, kind)
    assert pn.planes.shape == (p + 3, R.T, R.LDA) and pn.words.shape == (2, R.LDA)
    used = list(pn.cols) + [pn.ycol]
    assert len(set(used)) == p + 1
    out = ~pn.rows
    for k in used:
        assert np.isfinite(pn.planes[k][pn.rows]).all()
        bad = pn.planes[k][out]
        assert (~np.isfinite(bad) | (bad == 1e308)).all()
        assert np.isnan(bad).any() and (bad == np.inf).any() and (bad == -np.inf).any()
    for k in set(range(p + 3)) - set(used):
        assert np.isnan(pn.planes[k]).all()
    # the row set: bit set, a < A_END, a date in range -- and bits are set outside it as well
    tt, aa = np.nonzero(pn.rows)
    assert aa.max() < R.A_END and tt.min() == R.T0 and tt.max() == R.T0 + R.NT - 1
    assert pn.keep[pn.rows].all()
    assert pn.keep[:, R.A_END:].any() and pn.keep[:R.T0].any() and pn.keep[R.T0 + R.NT:].any()
    assert not pn.rows[R.EMPTY_DATE].any() and not pn.rows[:, R.EMPTY_ASSET].any()
    assert R.T0 < R.EMPTY_DATE < R.T0 + R.NT and 64 <= R.EMPTY_ASSET < 128
    assert 0.7 < pn.rows[R.T0:R.T0 + R.NT, :R.A_END].mean() < 0.85
    # statistics: NaN exactly on the assets without a row
    norow = ~pn.rows.any(axis=0)
    assert norow[R.EMPTY_ASSET] and norow[R.A_END:].all() and norow.sum() == R.LDA - R.A_END + 1
    assert np.isnan(pn.zs[:, norow]).all() and np.isfinite(pn.zs[:, ~norow]).all()
    assert (pn.zs[p, ~norow] == [0.0, 1.0]).all()
    # the words are the bits as passed
    for t in (0, 31, 32, 63, 64, 69):
        bit = (pn.words[t // 64] >> np.uint64(t % 64)) & np.uint64(1)
        assert np.array_equal(bit.astype(bool), pn.keep[t])


@pytest.mark.parametrize("kind", ["real", "int"])
@pytest.mark.parametrize("raw", [False, True])
def test_ref_sums_its_groups(kind, raw):
    """Panel.ref over (date, row-block) groups against one Gram over the same rows."""
    pn = R.make_panel(14, kind)
    t0, t1, a0, a1 = 31, 66, 64, 256                          # a1 past LDA: clipped
    sel = np.zeros_like(pn.rows)
    sel[t0:t1, a0:a1] = pn.rows[t0:t1, a0:a1]
    D = pn.design(*np.nonzero(sel), raw=raw)
    G, M, n = pn.ref(t0, t1, a0, a1, raw=raw)
    Ge, Me, ne = R.gram_exact(D)
    assert n == ne == sel.sum() and G[0, 0] == n
    if kind == "int":
        assert M is None and np.array_equal(G.astype(R.LD), Ge)
    else:
        eps = np.finfo(R.LD).eps
        assert (np.abs(G - Ge) <= n * eps * Me).all() and (np.abs(M - Me) <= n * eps * Me).all()
    G0, _, n0 = pn.ref(R.EMPTY_DATE, R.EMPTY_DATE + 1, 0, 192, raw=raw)
    assert n0 == 0 and not G0.any()


def test_scattered_stats_and_zplanes():
    p = 15
    pn = R.make_panel(p, "real")
    zs, zcols, zid = R.scattered_stats(pn)
    assert zs.shape == (p + 5, R.LDA, 2) and len(set(zcols)) == p and zid not in zcols
    assert 0 < zid < p + 4 and not np.array_equal(zcols, np.arange(p))
    nat = np.concatenate([zs[zcols], zs[zid][None]])
    assert np.array_equal(nat.view(np.int64), pn.zs.view(np.int64))
    rest = np.setdiff1d(np.arange(p + 5), list(zcols) + [zid])
    assert len(rest) == 4 and np.isnan(zs[rest]).all()
    zp = pn.zplanes()
    tt, aa = np.nonzero(pn.rows)
    D = pn.design(tt, aa)
    assert np.array_equal(zp[:, tt, aa], D[1:])
    assert not np.isfinite(zp[:, ~pn.rows][np.abs(zp[:, ~pn.rows]) != 1e308]).any()


def test_zpredict_seq():
    rng = np.random.default_rng(3)
    p, n = 65, 200
    x, mu = rng.normal(size=(p, n)), rng.normal(size=(p, 1))
    rs = 1.0 / rng.uniform(0.5, 3.0, size=(p, 1))
    beta = rng.normal(size=p + 1)
    zero = rng.random(p) < 0.7
    beta[1:][zero] = 0.0
    beta[1 + np.flatnonzero(zero)[0]] = -0.0
    xp = x.copy()
    xp[zero] = np.nan                                      # skipped columns are never read
    s = R.zpredict_seq(beta, xp, mu, rs)
    z = (x - mu) * rs
    ld = R.LD(beta[0]) + (beta[1:, None].astype(R.LD) * z.astype(R.LD)).sum(axis=0)
    mag = np.abs(beta[0]) + (np.abs(beta[1:, None]) * np.abs(z)).sum(axis=0)
    assert np.isfinite(s).all() and (np.abs(s - ld) <= (p + 1) * R.U * mag).all()
    only_b0 = 2.5 * (np.arange(p + 1) == 0)                 # all-zero coefficients: pred = beta[0]
    assert np.array_equal(R.zpredict_seq(only_b0, xp, mu, rs), np.full(n, 2.5))
