"""CPU pins of tests/analyzer_ref.py: every numpy restatement the direct kernel tests compare
with equals the pandas statement of the reference it stands for, bit for bit, on the tests' own
inputs -- including dates and groups of more than 8192 rows, where numpy's sum is not one pairwise
tree.  Also: the multi-buffer cases do tell the buffered reduction from a single tree."""
import numpy as np
import pytest

import analyzer_ref as R
from helpers import same


def test_fwd_returns_ref_is_pct_change_shift():
    close, present = R.fwd_inputs()
    fr = R.fwd_returns_ref(close, present)
    assert np.isnan(fr[:, ~present]).all()
    for a in range(close.shape[1]):
        days = np.flatnonzero(present[:, a])
        for q, k in enumerate(R.KS):
            assert same(fr[q, days, a], R.fwd_returns_pandas(close[days, a], k)), (a, k)
    # the cases the inputs are there for
    assert fr[0, 60, 5] == 1.0 and np.isnan(fr[1, 60, 5]) and not np.isnan(fr[0, 61, 5])
    assert close[62, 5] / close[60, 5] - 1 == 1 + 2.0 ** -51
    assert fr[0, 62, 2] == close[193, 2] / close[62, 2] - 1 or np.isnan(fr[0, 62, 2])
    assert same(fr[0, [63, 64, 127, 128], 1] <= 1, [True, True, True, False])
    assert np.isnan(fr[:, :, 4]).all()


@pytest.mark.parametrize("A,lda", [(20001, 20032), (70, 128), (3, 64)])
def test_prepare_ref_is_merge_dropna_demean(A, lda):
    sig, fr = R.prepare_inputs(A, lda)
    ref = R.prepare_ref(sig[:, :A], fr[:, :, :A])
    assert [len(i) for i, _ in ref] == [min(c, A) for c in R.PREP_COUNTS]
    for t, (idx, rows) in enumerate(ref):
        pidx, prows = R.prepare_pandas(sig[t, :A], fr[:, t, :A])
        assert same(idx, pidx) and same(rows, prows), t


@pytest.mark.parametrize("A,lda", [(32768, 32768), (20001, 20032)])
def test_prepare_inputs_tell_buffered_reduce_from_one_tree(A, lda):
    """On every date with more than 8192 surviving rows at least one of the three means differs
    between numpy's buffered reduction and a single pairwise tree; and the three step masks
    differ wherever rows are left over."""
    sig, fr = R.prepare_inputs(A, lda)
    seen = 0
    for t in range(sig.shape[0]):
        keep = ~np.isnan(sig[t, :A])
        ns, differs = [], []
        for q in range(3):
            keep = keep & ~np.isnan(fr[q, t, :A])
            v = np.ascontiguousarray(fr[q, t, :A][keep])
            ns.append(len(v))
            if len(v) > R.NP_BUF:
                differs.append(R.one_tree_sum(v) / len(v) != R.np_mean(v))
        if ns[2] < A and A - ns[2] >= 16:
            assert ns[0] > ns[1] > ns[2], (t, ns)
        if ns[2] > R.NP_BUF:
            seen += 1
            assert any(differs), (t, ns)
    assert seen == 3                                   # 8193, 16385 and the full width


@pytest.mark.parametrize("kind", ["normal", "ties", "zeros", "inf"])
def test_rank_ref_is_rank_first(kind):
    v = R.rank_values(np.random.default_rng(3), kind, (5, 300))
    for t in range(5):
        ra, rd = R.rank_ref(v[t])
        pa, pd_ = R.rank_pandas(v[t])
        assert same(ra, pa) and same(rd, pd_), t


def test_fill_refs_are_fillna_mean():
    planes, present = R.date_fill_inputs(20001, 20032)
    want = R.date_mean_fill_ref(planes, present)
    assert same(want[:, ~present], planes[:, ~present])
    for t in range(planes.shape[1]):
        rows = np.flatnonzero(present[t])
        if len(rows):
            assert same(want[:, t, rows].T, R.date_mean_fill_pandas(planes[:, t, rows].T)), t
    assert same(want[0, 2], planes[0, 2]) and np.isnan(want[1, 3][present[3]]).all()


def test_group_demean_ref_is_series_mean():
    x, off = R.group_inputs()
    want = R.group_demean_ref(x, off)
    for g in range(len(off) - 1):
        assert same(want[off[g]:off[g + 1]], R.group_demean_pandas(x[off[g]:off[g + 1]])), g
    assert np.isnan(want[off[5]:off[6]]).all()
    big = x[off[9]:off[10]]
    bad = np.isnan(big)
    assert R.one_tree_sum(np.where(bad, 0.0, big)) / (~bad).sum() != R.np_nanmean(big)


def test_stats_pandas_agrees_with_oracle_on_finite_rows():
    """The pandas statements of the per-date statistics against the oracle, which the reference's
    goldens pin: IC and the top-10 returns, for pivots of 10, 9 and 2 columns."""
    from oracle import xs
    rows, counts = R.stats_inputs("finite")
    for sel in (range(10), range(3), range(2)):
        per = [rows[:, t, :counts[t]] for t in sel]
        ic, lm, lc, port = R.stats_pandas(per)
        date = np.concatenate([np.full(counts[t], i) for i, t in enumerate(sel)])
        vals = np.concatenate([p.T for p in per])
        d, tp, v = xs.top_stocks(date, vals)
        assert same(v.reshape(len(per), 6)[:, :3], port)
        od, ot, oic = xs.ic_series(date, vals)
        assert same(oic, ic[~np.isnan(ic)])
        assert same(lc.sum(axis=1), counts[list(sel)])
