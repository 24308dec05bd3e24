"""The references of the factor-screening tests (tests/screen_ref.py) pinned on the CPU: the
plain-Python restatement of pandas' nancorr recurrence and the one-frame form equal the per-column
pandas statement bit for bit on the inputs the GPU tests use, and the whole-sample statistics are
pandas' mean, std and their quotient."""
import numpy as np
import pandas as pd
import pytest

import screen_ref as S
from helpers import same

# every import of the tests in this file needs the screening interface
from afm import _lib  # noqa: F401

assert hasattr(_lib, "SIGNATURES_SCREEN")

PLANES = (0, 3, 5, 7, 64, 66, 70, 129)          # ties, inf in the last row, constant, ...


@pytest.mark.parametrize("kind", ["finite", "inf", "retinf"])
def test_restatement_and_wide_form_equal_the_pandas_statement(kind):
    """Per date and column: DataFrame.corr of [factor, three returns] == the recurrence in Python
    floats == the entry of the one-frame corr, on the finite, inf (first chunk, later chunk, last
    row), inf-in-one-return, constant-column, 1-row and 2-row cases."""
    planes, rows, rows_idx, nrows = S.screen_inputs(S.COUNTS_A, kind)
    wide = S.screen_ref(planes, rows, rows_idx, nrows)
    seen_nan = seen_val = 0
    for t, n in enumerate(nrows):
        if n == 0:
            assert np.isnan(wide[t]).all()
            continue
        idx = rows_idx[t, :n]
        for p in PLANES:
            f, rets = planes[p, t, idx], rows[1:, t, :n]
            want = S.ic_pandas(f, rets)
            assert same(S.ic_recurrence(f, rets), want), (kind, t, p)
            assert same(wide[t, p], want), (kind, t, p)
            seen_nan += int(np.isnan(want).sum())
            seen_val += int((~np.isnan(want)).sum())
    assert seen_nan and seen_val


def test_chunk_edge_counts_come_from_the_kernel_constants():
    rows, inv = S.kernel_constant("kScreenRows"), S.kernel_constant("kScreenInv")
    c = S.counts_chunk_edges()
    for e in (rows, 2 * rows, inv):
        assert {e - 1, e, e + 1} <= set(c)
    assert max(c) <= S.LDA


def test_z_reference_and_unusable_column():
    """With the {mu, 1/sd} table the reference is (x - mu) * inv in numpy; the {0, 0} row gives a
    constant 0 -> NaN IC on every date."""
    planes, rows, rows_idx, nrows = S.screen_inputs(S.COUNTS_A[:6], "finite")
    zs = S.zs_table(planes.shape[0])
    ic = S.screen_ref(planes, rows, rows_idx, nrows, zs)
    assert np.isnan(ic[:, 7]).all() and not np.isnan(ic[2:, 6]).any()
    t = 5
    idx = rows_idx[t, :nrows[t]]
    z = (planes[2, t, idx] - zs[2, idx, 0]) * zs[2, idx, 1]
    assert same(ic[t, 2], S.ic_pandas(z, rows[1:, t, :nrows[t]]))
    assert not same(ic[t, 2], S.screen_ref(planes, rows, rows_idx, nrows)[t, 2])


def test_summary_is_pandas_mean_std_quotient():
    rng = np.random.default_rng(5)
    year = np.repeat([2001, 2002, 2003], [1, 2, 40]).astype(np.int32)
    ic = rng.uniform(-1, 1, (len(year), 4, 3))
    ic[rng.random(ic.shape) < 0.1] = np.nan
    ic[:, 1, 0] = np.nan                                   # n = 0
    ic[1:, 1, 1] = np.nan                                  # n = 1
    stats, ir_year = S.summary_pandas(ic, year, 3, 2001)
    assert stats[1, 0, 0] == 0 and np.isnan(stats[1, 0, 1:]).all()
    assert stats[1, 1, 0] == 1 and stats[1, 1, 1] == ic[0, 1, 1] and np.isnan(stats[1, 1, 2:]).all()
    s = pd.Series(ic[:, 2, 2]).dropna()
    assert stats[2, 2, 0] == len(s) and stats[2, 2, 1] == s.mean() and stats[2, 2, 2] == s.std()
    assert stats[2, 2, 3] == s.mean() / s.std()
    assert stats[2, 2, 4] == s.mean() / s.std() * np.sqrt(float(len(s)))
    g = pd.Series(ic[3:, 0, 1]).dropna()
    assert ir_year[2, 0, 1] == g.mean() / g.std()
    assert np.isnan(ir_year[0]).all()                      # one date: std is NaN
