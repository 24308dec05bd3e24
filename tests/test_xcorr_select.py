"""``afm.screen.select_factors`` on hand-made score vectors and matrices (no library, no GPU):
greedy by |score| descending, stable in column order, NaN scores left out, a NaN correlation
counts as 0, stop at k."""
import numpy as np
import pytest

from afm.screen import select_factors


def invariants(names, score, corr, max_corr, kept):
    """Every kept pair is <= max_corr; every candidate skipped ahead of the last kept one has a
    kept, better-scored (earlier in the walk) partner above max_corr."""
    s = np.abs(np.asarray(score, dtype=float))
    c = np.where(np.isnan(corr), 0.0, np.asarray(corr, dtype=float))
    walk = [i for i in sorted(range(len(names)), key=lambda i: (-s[i] if s[i] == s[i] else 0, i))
            if s[i] == s[i]]
    pos = {names[i]: w for w, i in enumerate(walk)}
    idx = {n: i for i, n in enumerate(names)}
    assert [pos[n] for n in kept] == sorted(pos[n] for n in kept)
    for a in kept:
        for b in kept:
            if a != b:
                assert c[idx[a], idx[b]] <= max_corr
    last = max((pos[n] for n in kept), default=0)
    for i in walk[:last]:
        if names[i] not in kept:
            assert any(pos[b] < pos[names[i]] and c[i, idx[b]] > max_corr for b in kept)


NAMES = list("abcdef")
SCORE = np.array([0.5, -0.9, 0.9, np.nan, 0.2, -0.5])       # ties: b / c and a / f
CORR = np.array([[1.0, 0.1, 0.2, 0.0, 0.8, 0.75],
                 [0.1, 1.0, 0.95, 0.3, np.nan, 0.2],
                 [0.2, 0.95, 1.0, 0.1, 0.3, 0.1],
                 [0.0, 0.3, 0.1, 1.0, 0.0, 0.0],
                 [0.8, np.nan, 0.3, 0.0, 1.0, 0.1],
                 [0.75, 0.2, 0.1, 0.0, 0.1, 1.0]])


def test_ties_nan_scores_and_nan_correlations():
    # walk: b, c (tie, column order), a, f (tie), e; d has no score
    got = select_factors(NAMES, SCORE, CORR, max_corr=0.7)
    assert got == ["b", "a"]               # c ~ b (0.95); f ~ a (0.75); e ~ a (0.8)
    invariants(NAMES, SCORE, CORR, 0.7, got)
    # e's NaN correlation with b counts as 0: at 0.85 only c is too close to what is kept
    assert select_factors(NAMES, SCORE, CORR, max_corr=0.85) == ["b", "a", "f", "e"]
    # the sign of the score does not matter, the column order breaks the ties
    # reversed columns: c before b, f before a; a goes (0.75 with f), so e stays
    assert select_factors(NAMES[::-1], SCORE[::-1], CORR[::-1, ::-1], max_corr=0.7) == \
        ["c", "f", "e"]


def test_default_threshold_and_the_walk():
    got = select_factors(NAMES, SCORE, CORR)
    invariants(NAMES, SCORE, CORR, 0.7, got)
    assert got[0] == "b" and "d" not in got and "c" not in got and "f" not in got


@pytest.mark.parametrize("max_corr", [0.0, 0.05, 0.15, 0.25, 0.7, 0.78, 0.9, 0.95, 1.0])
@pytest.mark.parametrize("k", [None, 0, 1, 2, 3, 5, 6, 10])
def test_invariants_over_thresholds_and_k(max_corr, k):
    full = select_factors(NAMES, SCORE, CORR, max_corr=max_corr)
    invariants(NAMES, SCORE, CORR, max_corr, full)
    got = select_factors(NAMES, SCORE, CORR, max_corr=max_corr, k=k)
    assert got == (full if k is None else full[:k])          # k smaller and larger than survives
    invariants(NAMES, SCORE, CORR, max_corr, got)


def test_a_threshold_that_keeps_everything_and_one_that_keeps_the_first():
    assert select_factors(NAMES, SCORE, CORR, max_corr=1.0) == ["b", "c", "a", "f", "e"]
    dense = np.full((6, 6), 0.5)
    assert select_factors(NAMES, SCORE, dense, max_corr=0.4) == ["b"]
    assert select_factors(NAMES, SCORE, dense, max_corr=0.5) == ["b", "c", "a", "f", "e"]
    assert select_factors(NAMES, np.full(6, np.nan), dense) == []
    assert select_factors([], [], np.zeros((0, 0))) == []


def test_random_matrices_keep_the_invariants():
    rng = np.random.default_rng(9)
    for trial in range(40):
        K = int(rng.integers(1, 25))
        names = [f"f{i}" for i in range(K)]
        score = np.round(rng.normal(size=K), 1)               # rounded: ties
        score[rng.random(K) < 0.1] = np.nan
        c = rng.random((K, K))
        c = (c + c.T) / 2
        c[rng.random((K, K)) < 0.1] = np.nan
        c = np.where(np.isnan(c.T), np.nan, c)
        thr = float(rng.choice([0.3, 0.5, 0.7]))
        k = None if trial % 3 else int(rng.integers(0, K + 2))
        got = select_factors(names, score, c, max_corr=thr, k=k)
        invariants(names, score, c, thr, got)
        assert len(set(got)) == len(got) and (k is None or len(got) <= k)
        assert got == select_factors(names, -score, c, max_corr=thr, k=k)   # |score|


def test_shape_errors():
    with pytest.raises(ValueError):
        select_factors(NAMES, SCORE[:5], CORR)
    with pytest.raises(ValueError):
        select_factors(NAMES, SCORE, CORR[:5])
    with pytest.raises(ValueError):
        select_factors(NAMES, SCORE, CORR, k=-1)
