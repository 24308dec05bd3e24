"""afm_zpredict_f64 called directly, bit for bit against the sequential restatement of
tests/zgram_ref.py (s = beta[0], then s = s + beta[1+j] * ((x - mu) * rs) over the non-zero
coefficients, ascending j): the ballot compaction at p = 0, 1, 63, 64, 65, 127 and 128 (64
coefficients per round), a date range that is no multiple of the workgroup's 4 dates and crosses
bit 32 and bit 64 of the presence words, and sparse, all-zero and dense coefficient vectors.

Every zero coefficient (-0.0 included) sits on a column whose statistics are NaN and whose plane
is NaN / +-inf / 1e308 everywhere, and every cell without a row is poisoned in every plane, so a
kernel that multiplies by a zero coefficient or reads a cell it must skip predicts a non-finite
value."""
import numpy as np
import pytest

import zgram_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FF8DEAD0000BEEF                  # the prefill: a NaN payload no kernel writes
T, LDA, T0, NT = 70, 128, 29, 37
EMPTY_ASSET = 5


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _beta(rng, p, case):
    beta = rng.normal(size=p + 1)
    beta[np.abs(beta) < 0.05] = 0.5
    if case == "zero":
        beta[1:] = 0.0
    elif case == "sparse" and p:
        zero = rng.random(p) < 0.7
        zero[[j for j in (0, 63, 64, p - 1) if j < p]] = False     # the edges of a ballot round
        zero[1:3] = p > 3
        beta[1:][zero] = 0.0
    if case != "dense" and p:
        beta[1 + np.flatnonzero(beta[1:] == 0.0)[::2]] = -0.0      # every other zero is -0.0
    return beta


def _case(p, case):
    rng = np.random.default_rng([17, p, ("sparse", "zero", "dense").index(case)])
    ncol = p + 2                                                # two unused planes, all NaN
    perm = rng.permutation(ncol)
    cols = perm[:p].astype(np.int32)
    beta = _beta(rng, p, case)
    keep = rng.random((T, LDA)) < 0.75                          # bits outside the range too
    keep[:, EMPTY_ASSET] = False
    rows = keep.copy()
    rows[:T0] = False
    rows[T0 + NT:] = False
    mu = rng.normal(4.0, 3.0, size=(p, LDA))
    sd = rng.uniform(0.5, 20.0, size=(p, LDA))
    planes = np.full((ncol, T, LDA), np.nan)
    planes[cols] = mu[:, None, :] + sd[:, None, :] * rng.normal(size=(p, T, LDA))
    zs = np.stack([mu, 1.0 / sd], axis=-1) if p else np.zeros((1, LDA, 2))
    zs[:, ~rows.any(axis=0)] = np.nan                           # the asset without rows
    for j in range(p):
        skipped = beta[1 + j] == 0.0
        if skipped:
            zs[j] = np.nan
        R.poison_cells(planes[cols[j]], np.ones_like(rows) if skipped else ~rows, phase=j)
    return dict(p=p, beta=beta, cols=cols, planes=planes, zs=zs, keep=keep, rows=rows)


def _reference(c):
    """pred over the dates [T0, T0 + NT) by the sequential loop (skipped columns are never read)"""
    x = c["planes"][c["cols"]][:, T0:T0 + NT]
    with np.errstate(all="ignore"):
        return R.zpredict_seq(c["beta"], x, c["zs"][:, None, :, 0], c["zs"][:, None, :, 1])


@pytest.mark.parametrize("case", ["sparse", "zero", "dense"])
@pytest.mark.parametrize("p", [0, 1, 63, 64, 65, 127, 128])
def test_zpredict(p, case):
    import torch
    from afm import _lib
    c = _case(p, case)
    beta, rows = c["beta"], c["rows"]
    nz = beta[1:] != 0.0
    if case == "sparse" and p >= 63:                             # about 70 % zeros of both signs
        zeros = beta[1:][~nz]
        assert 0.55 < 1 - nz.mean() < 0.85
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()
        assert nz[min(p, 64) - 1] and nz[p - 1]
    elif case != "sparse":
        assert nz.all() if case == "dense" else not nz.any()
    for j in np.flatnonzero(~nz):                                # zero coefficient: all poison
        assert np.isnan(c["zs"][j]).all() and not np.isfinite(
            c["planes"][c["cols"][j]][np.abs(c["planes"][c["cols"][j]]) != 1e308]).any()
    ref = _reference(c)
    assert np.isfinite(ref[rows[T0:T0 + NT]]).all()
    if case == "zero":
        assert (ref[rows[T0:T0 + NT]] == beta[0]).all()

    pred = torch.full((T, LDA), SENT, dtype=torch.int64, device="cuda").view(torch.float64)
    cols = _cuda(c["cols"] if p else np.zeros(1, dtype=np.int32))
    _lib.run("afm_zpredict_f64", _cuda(c["planes"]), T * LDA, LDA, T0, NT, cols, p, _cuda(c["zs"]),
             _cuda(beta), _cuda(R.pack_words(c["keep"]).view(np.int64)), pred)
    torch.cuda.synchronize()
    got = pred.cpu().numpy()
    inside = got[T0:T0 + NT]
    on = rows[T0:T0 + NT]
    assert np.isfinite(inside[on]).all()
    bad = np.argwhere((inside.view(np.int64) != ref.view(np.int64)) & on)
    assert len(bad) == 0, ("date/asset", T0 + bad[0][0], bad[0][1], inside[tuple(bad[0])],
                           ref[tuple(bad[0])])
    assert np.isnan(inside[~on]).all()                           # dates in range, no bit: NaN
    outside = np.r_[got[:T0], got[T0 + NT:]].view(np.int64)
    assert (outside == SENT).all()                               # other dates: untouched


def test_zpredict_rejects_p_129():
    import torch
    from afm import _lib
    p = 129
    planes = torch.zeros((1, T, LDA), dtype=torch.float64, device="cuda")
    cols = torch.zeros(p, dtype=torch.int32, device="cuda")
    zs = torch.ones((p, LDA, 2), dtype=torch.float64, device="cuda")
    beta = torch.ones(p + 1, dtype=torch.float64, device="cuda")
    bits = torch.zeros((2, LDA), dtype=torch.int64, device="cuda")
    pred = torch.full((T, LDA), SENT, dtype=torch.int64, device="cuda").view(torch.float64)
    with pytest.raises(_lib.AfmError, match="afm_zpredict_f64"):
        _lib.run("afm_zpredict_f64", planes, T * LDA, LDA, T0, NT, cols, p, zs, beta, bits, pred)
    torch.cuda.synchronize()
    assert (pred.view(torch.int64) == SENT).all().item()
