"""afm_screen_turnover_f64 and afm_screen_turnover_summary_f64 (csrc/turnover.hip) called directly
on hand-built planes, every output filled with a sentinel first: bit for bit tests/turnover_ref.py
(pinned against pandas on the CPU by tests/test_turnover_ref.py) on every output.

The marks kernel's constants the row counts below are named from: kTvThreads = 1024 rows of one
chunk of the method='first' scan; kTvFewKeys * kTvThreads = 4096 and kTvMidKeys * kTvThreads =
16384 rows, the capacities of its first two instantiations (the third holds 32768 = the lda
limit); kTvLdsRows = 16384 rows sort in LDS, more through the scratch; kTvBudget = 128 MiB of date
slots in the scratch, beyond which the dates are taken in blocks."""
import ctypes
import functools

import numpy as np
import pytest

import turnover_ref as R
from helpers import same

pytestmark = pytest.mark.gpu

SENT = -7.25
ISENT = -7


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).to(torch.device("cuda", 0))   # (a writable copy)


def run(name, *args):
    from afm import _lib
    return _lib.run(name, *args)


def turnover(planes, cols, rows_idx, nrows, dates, lags, zs=None, zcols=None, extra=1):
    """The call on host inputs -> rank_ac, counts, port_turn [nd]...; ``extra`` sentinel rows past
    nd must come back untouched."""
    import torch
    _, T, lda = planes.shape
    nd, K, L = len(dates), len(cols), len(lags)
    opt = dict(dtype=torch.float64, device="cuda:0")
    ac = torch.full((nd + extra, K, L), SENT, **opt)
    cnt = torch.full((nd + extra, K, L, 5), ISENT, dtype=torch.int32, device="cuda:0")
    pt = torch.full((nd + extra, K, L), SENT, **opt)
    nbytes = run("afm_screen_turnover_scratch_bytes", nd, K, lda)
    scr = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda:0")
    run("afm_screen_turnover_f64", dev(planes), T * lda, T, lda, dev(np.asarray(cols, np.int32)), K,
        None if zs is None else dev(zs), None if zcols is None else dev(np.asarray(zcols, np.int32)),
        dev(np.asarray(dates, np.int32)), nd, dev(rows_idx), dev(nrows),
        (ctypes.c_int32 * L)(*lags), L, ac, cnt, pt, scr)
    ac, cnt, pt = ac.cpu().numpy(), cnt.cpu().numpy(), pt.cpu().numpy()
    assert (ac[nd:] == SENT).all() and (cnt[nd:] == ISENT).all() and (pt[nd:] == SENT).all()
    return ac[:nd], cnt[:nd], pt[:nd]


def check(got, want, what=""):
    for g, w, name in zip(got, want, ("rank_ac", "counts", "port_turn")):
        assert same(g, w), (what, name, np.argwhere(~((g == w) | ((g != g) & (w != w))))[:5])


def random_rows(rng, T, lda, counts):
    mask = np.zeros((T, lda), dtype=bool)
    for t, n in enumerate(counts):
        mask[t, rng.permutation(lda)[:n]] = True
    return mask


# ---- the small planes ------------------------------------------------------------------------------
COUNTS = [9, 1, 2, 10, 0, 11, 63, 64, 65, 12, 30, 128]      # a date without rows in the middle
KINDS = ["distinct", "ties", "const", "special"]
LAGS = (1, 2, 11)


@functools.lru_cache(maxsize=None)
def small():
    """planes [4][12][128] (KINDS), rows_idx, nrows and the reference of all dates at LAGS."""
    rng = np.random.default_rng(11)
    T, lda = len(COUNTS), 128
    x = np.empty((4, T, lda))
    x[0] = rng.standard_normal((T, lda))
    x[1] = rng.integers(0, 15, (T, lda)) - 7.0              # 15 values
    x[2] = 2.5
    x[3] = np.round(rng.standard_normal((T, lda)) * 2) / 2
    sp = rng.random((T, lda))
    x[3][sp < 0.15] = np.nan
    x[3][(sp >= 0.15) & (sp < 0.20)] = np.inf
    x[3][(sp >= 0.20) & (sp < 0.25)] = -np.inf
    x[3][(sp >= 0.25) & (sp < 0.35)] = -0.0
    x[3][(sp >= 0.35) & (sp < 0.45)] = 0.0
    rows_idx, nrows = R.rows_of(random_rows(rng, T, lda, COUNTS))
    ref = R.turnover(x, rows_idx, nrows, np.arange(T), LAGS)
    for a in (x, rows_idx, nrows) + ref:
        a.setflags(write=False)
    return x, rows_idx, nrows, ref


def test_row_counts_values_and_lags_on_the_small_planes():
    x, rows_idx, nrows, ref = small()
    T = x.shape[1]
    got = turnover(x, [0, 1, 2, 3], rows_idx, nrows, np.arange(T), LAGS)
    check(got, ref)
    ac, cnt, pt = got
    assert np.isnan(ac[:, 2]).all()                          # the constant column has no spread
    assert np.isfinite(ac[2:, 0, 0]).sum() >= 5
    assert (cnt[5:, :3, 0, 1] > 0).all()                     # a ranked date has a layer 10
    one = turnover(x, [0, 1, 2, 3], rows_idx, nrows, np.arange(T), (1,))
    check(one, [a[:, :, :1] for a in ref], "lags (1,)")


def test_a_lag_past_the_dates_and_a_repeated_lag():
    x, rows_idx, nrows, ref = small()
    T = x.shape[1]
    ac, cnt, pt = turnover(x, [0, 3], rows_idx, nrows, np.arange(T), (2, T, 2, T + 5))
    for l in (1, 3):                                         # everything empty
        assert np.isnan(ac[:, :, l]).all() and np.isnan(pt[:, :, l]).all()
        assert (cnt[:, :, l] == 0).all()
    for a, r in zip((ac, cnt, pt), ref):
        assert same(a[:, :, 0], r[:, [0, 3], 1]) and same(a[:, :, 2], a[:, :, 0])


@pytest.mark.parametrize("K", [1, 3, 65])
def test_column_counts_and_repeated_columns(K):
    x, rows_idx, nrows, ref = small()
    T = x.shape[1]
    cols = [(3 * k + 1) % 4 for k in range(K)]               # every plane, named again and again
    got = turnover(x, cols, rows_idx, nrows, np.arange(T), LAGS)
    check(got, [r[:, cols] for r in ref], K)


def test_z_path_equals_the_raw_plane_of_the_same_z_values():
    x, rows_idx, nrows, _ = small()
    rng = np.random.default_rng(5)
    T, lda = x.shape[1:]
    zs = np.empty((3, lda, 2))
    zs[:, :, 0] = rng.standard_normal((3, lda))
    zs[:, :, 1] = 1.0 / (0.5 + rng.random((3, lda)))
    cols, zcols = [3, 0, 1], [2, 0, 1]
    z = np.stack([(x[c] - zs[r, :, 0][None, :]) * zs[r, :, 1][None, :]
                  for c, r in zip(cols, zcols)])
    dates = np.arange(T)
    via_zs = turnover(x, cols, rows_idx, nrows, dates, (1, 2), zs=zs, zcols=zcols)
    raw = turnover(z, [0, 1, 2], rows_idx, nrows, dates, (1, 2))
    check(via_zs, raw, "zs against the raw z plane")
    check(raw, R.turnover(z, rows_idx, nrows, dates, (1, 2)), "raw z plane")
    rowk = turnover(x, [0, 1, 3], rows_idx, nrows, dates, (1,), zs=zs)       # zcols NULL: row k
    z2 = np.stack([(x[c] - zs[k, :, 0][None, :]) * zs[k, :, 1][None, :]
                   for k, c in enumerate([0, 1, 3])])
    check(rowk, R.turnover(z2, rows_idx, nrows, dates, (1,)), "zcols NULL")


def test_dates_need_not_be_contiguous_and_an_item_depends_on_its_two_dates_alone():
    x, rows_idx, nrows, ref = small()
    dates = np.array([0, 2, 3, 5, 6, 8, 9, 11])
    got = turnover(x, [0, 1, 2, 3], rows_idx, nrows, dates, (1, 3))
    check(got, R.turnover(x, rows_idx, nrows, dates, (1, 3)), "dates with gaps")
    # the full run's items again with another K, other neighbours, other lags around them and the
    # positions shifted
    shifted = np.arange(3, 12)
    for cols, lags in (([2, 0], (2, 1)), ([3], (5, 11, 1, 2)), ([1, 1, 3, 0, 2], (2,))):
        got = turnover(x, cols, rows_idx, nrows, shifted, lags)
        for l, lag in enumerate(lags):
            if lag not in LAGS:
                continue
            for a, r in zip(got, ref):
                assert same(a[lag:, :, l], r[3 + lag:, cols, LAGS.index(lag)]), (cols, lags, lag)


def test_layer_counts_equal_the_layers_kernel():
    import torch
    x, rows_idx, nrows, _ = small()
    _, T, lda = x.shape
    _, cnt, _ = turnover(x, [0, 1, 2, 3], rows_idx, nrows, np.arange(T), (1,))
    opt = dict(dtype=torch.float64, device="cuda:0")
    lm = torch.empty((T, 4, 3, 10), **opt)
    lc = torch.empty((T, 4, 10), dtype=torch.int32, device="cuda:0")
    port = torch.empty((T, 4, 3), **opt)
    run("afm_screen_layers_f64", dev(x), T * lda, T, lda, dev(np.arange(4, dtype=np.int32)), 4,
        None, None, dev(np.arange(T, dtype=np.int32)), T, torch.zeros((4, T, lda), **opt),
        dev(rows_idx), dev(nrows), lm, lc, port, torch.empty(T * 4 * 40 + 4, **opt))
    lc = lc.cpu().numpy()
    assert (cnt[1:, :, 0, 1] == lc[1:, :, 9]).all() and (cnt[1:, :, 0, 3] == lc[1:, :, 0]).all()


# ---- row sets --------------------------------------------------------------------------------------
def test_row_sets_identical_nested_one_shared_disjoint_and_empty():
    rng = np.random.default_rng(3)
    T, lda = 8, 64
    sets = [range(0, 20), range(0, 20), range(0, 40), range(39, 59), range(0, 20), (),
            range(0, 20), range(5, 31)]
    mask = np.zeros((T, lda), dtype=bool)
    for t, s in enumerate(sets):
        mask[t, list(s)] = True
    rows_idx, nrows = R.rows_of(mask)
    x = np.stack([rng.standard_normal((T, lda)), rng.integers(0, 4, (T, lda)).astype(np.float64)])
    x[:, 1] = x[:, 0]                                        # the identical pair: rows and values
    for lags in ((1,), (1, 2, T - 1)):
        got = turnover(x, [0, 1], rows_idx, nrows, np.arange(T), lags)
        check(got, R.turnover(x, rows_idx, nrows, np.arange(T), lags), lags)
    ac, cnt, pt = got
    assert (ac[1, :, 0] == 1.0).all() and (cnt[1, :, 0, [2, 4]] == 0).all()   # identity
    assert (pt[1, :, 0] == 0.0).all() and (cnt[1, :, 0, 0] == 20).all()
    assert (cnt[3, :, 0, 0] == 1).all() and np.isnan(ac[3, :, 0]).all()       # one shared asset
    assert (cnt[4, :, 0, 0] == 0).all()                                         # disjoint
    assert (cnt[4, :, 0, 2] == cnt[4, :, 0, 1]).all()       # an asset off the earlier date is new
    assert (cnt[5] == 0).all() and np.isnan(pt[5]).all() and np.isnan(pt[6, :, 0]).all()


# ---- method='first' at the three bounds ------------------------------------------------------------
def test_ties_straddling_the_layer_bounds_and_the_tenth_largest():
    """25 ranked rows: layer 1 ends at first-rank 2, layer 10 starts at 23, the book ends at
    first-rank 16 from below.  Pairs of equal values sit on ranks (2, 3), (15, 16, 17) and (22, 23,
    24), their rows in a new order on every date, so row position alone decides."""
    rng = np.random.default_rng(17)
    T, lda, n = 8, 64, 25
    base = np.arange(1.0, n + 1)
    base[2] = base[1]
    base[15] = base[16] = base[14]
    base[22] = base[23] = base[21]
    x = np.full((3, T, lda), np.nan)
    mask = np.zeros((T, lda), dtype=bool)
    for t in range(T):
        a = np.sort(rng.permutation(lda)[:n])
        mask[t, a] = True
        x[0, t, a] = base[rng.permutation(n)]
        x[1, t, a] = -base[rng.permutation(n)]              # the same from the other end
        x[2, t, a] = base[rng.permutation(n)] - 16.0        # mixed signs in the book
    rows_idx, nrows = R.rows_of(mask)
    got = turnover(x, [0, 1, 2], rows_idx, nrows, np.arange(T), (1, 3))
    ref = R.turnover(x, rows_idx, nrows, np.arange(T), (1, 3))
    check(got, ref)
    assert (ref[1][1:, :, 0, 1] == 3).all() and (ref[1][1:, :, 0, 3] == 2).all()
    m = R.marks(x[0, 0], rows_idx[0][:n])
    tied = {int(a) for a in rows_idx[0][:n] if x[0, 0, a] == base[21]}
    assert len(tied & m[1]) == 2 and len(tied - m[1]) == 1  # the tie is split by the bound


def test_special_values_in_the_book_and_a_column_missing_on_the_earlier_date():
    T, lda = 6, 64
    x = np.full((4, T, lda), np.nan)
    mask = np.zeros((T, lda), dtype=bool)
    mask[:, :24] = True
    rows_idx, nrows = R.rows_of(mask)
    rng = np.random.default_rng(2)
    low = -10.0 - np.arange(14.0)
    for t in range(T):
        x[0, t, :24] = rng.permutation(np.r_[[5, 4, 3, 2, 1, -1, -2, -3, -4, -5.0], low])  # sums to 0
        x[1, t, :24] = rng.permutation(np.r_[[5, 4, 3, 2, 1, -1, -2, -3, -4, -4.0], low])  # to 1
        x[2, t, :24] = rng.permutation(np.r_[[-0.0] * 6, [0.0] * 6, -np.arange(1.0, 13)])   # +-0
        x[3, t, :24] = rng.standard_normal(24)
    x[3, 2, :] = np.nan                                      # all-NaN on one date
    x[3, 4, :20] = np.nan                                    # four ranked rows
    got = turnover(x, [0, 1, 2, 3], rows_idx, nrows, np.arange(T), (1, 2))
    ref = R.turnover(x, rows_idx, nrows, np.arange(T), (1, 2))
    check(got, ref)
    ac, cnt, pt = got
    assert np.isnan(pt[1:, 0, 0]).all() and np.isfinite(pt[1:, 1, 0]).all()
    assert np.isnan(pt[1:, 2, 0]).all()                      # a book of zeros has no weights
    assert cnt[3, 3, 0, 0] == 0 and cnt[3, 3, 0, 1] == cnt[3, 3, 0, 2] > 0   # t0 all-NaN: all new
    assert cnt[2, 3, 0, 1] == 0 and np.isnan(pt[2, 3, 0]) and np.isnan(pt[3, 3, 0])


# ---- many rows: every instantiation, the scan over chunks, the sort through the scratch ------------
@pytest.mark.parametrize("n, lda", [(1025, 1088), (4096, 4096), (4097, 4160), (16384, 16384),
                                    (16385, 16448), (32768, 32768)])
def test_many_rows(n, lda):
    rng = np.random.default_rng(n)
    x = np.round(rng.standard_normal((1, 2, lda)) * 300) / 4   # ties of many sizes
    x[0, :, rng.permutation(lda)[:lda // 50]] = np.nan
    # a tie that crosses the chunks of the scan sits on each bound
    order = np.argsort(x[0, 1], kind="stable")
    nk = int((~np.isnan(x[0, 1])).sum())
    for r in (nk // 10, nk - nk // 10, nk - 10):
        x[0, 1, order[max(r - 40, 0):r + 40]] = x[0, 1, order[r]]
    mask = np.zeros((2, lda), dtype=bool)
    mask[0, rng.permutation(lda)[:max(n - 7, 1)]] = True
    mask[1, rng.permutation(lda)[:n]] = True
    rows_idx, nrows = R.rows_of(mask)
    got = turnover(x, [0], rows_idx, nrows, [0, 1], (1,))
    check(got, R.turnover(x, rows_idx, nrows, [0, 1], (1,)), (n, lda))
    assert np.isfinite(got[0][1, 0, 0]) and np.isfinite(got[2][1, 0, 0])


def test_dates_in_blocks_when_the_marks_exceed_the_scratch_budget():
    """4096 columns (four planes named again and again) of 64 assets are 1.8 MB of marks a date:
    the 128 MiB of slots hold 73 of the 96 dates, so lags 1 and 5 ride the ring in two blocks and
    lags 40 and 90 (past half the ring) are paired with both sides computed again."""
    rng = np.random.default_rng(8)
    T, lda, K = 96, 64, 4096
    x = np.round(rng.standard_normal((4, T, lda)) * 4) / 4
    x[rng.random(x.shape) < 0.05] = np.nan
    rows_idx, nrows = R.rows_of(rng.random((T, lda)) < 0.8)
    lags = (1, 5, 40, 90)
    assert run("afm_screen_turnover_scratch_bytes", T, K, lda) < \
        run("afm_screen_turnover_scratch_bytes", T, K // 2, lda) * 2
    ref = R.turnover(x, rows_idx, nrows, np.arange(T), lags)
    cols = np.arange(K) % 4
    ac, cnt, pt = turnover(x, cols, rows_idx, nrows, np.arange(T), lags)
    for a, r in zip((ac, cnt, pt), ref):
        assert same(a, r[:, cols])


# ---- errors ----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_written():
    import torch
    from afm import _lib
    x, rows_idx, nrows, _ = small()
    _, T, lda = x.shape
    opt = dict(dtype=torch.float64, device="cuda:0")
    ac = torch.full((T, 2, 2), SENT, **opt)
    cnt = torch.full((T, 2, 2, 5), ISENT, dtype=torch.int32, device="cuda:0")
    pt = torch.full((T, 2, 2), SENT, **opt)
    scr = torch.full((run("afm_screen_turnover_scratch_bytes", T, 2, lda) // 8,), -1,
                     dtype=torch.int64, device="cuda:0")

    def lags(*v):
        return (ctypes.c_int32 * max(len(v), 1))(*v)
    good = [dev(x), T * lda, T, lda, dev(np.array([0, 1], np.int32)), 2, None, None,
            dev(np.arange(T, dtype=np.int32)), T, dev(rows_idx), dev(nrows), lags(1, 2), 2, ac, cnt,
            pt, scr]

    def bad(msg, **kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        with pytest.raises(_lib.AfmError, match=msg) as e:
            run("afm_screen_turnover_f64", *a)
        assert "(-1)" in str(e.value)                        # AFM_E_ARG
    bad("lda", _3=96)
    bad("lda", _3=32768 + 64)
    bad("L must be in 1..8", _13=0)
    bad("L must be in 1..8", _12=lags(*range(1, 10)), _13=9)
    bad("lags", _12=lags(1, 0))
    bad("lags", _12=lags(-3, 2))
    bad("lags", _12=None)
    bad("K must be at least 1", _5=0)
    bad("nd is negative", _9=-1)
    bad("nd \\* K \\* L must be below 2\\^31", _9=1 << 30)
    bad("null buffer", _0=None)
    bad("null buffer", _17=None)
    bad("zcols without zs", _7=good[4])
    torch.cuda.synchronize()
    assert (ac == SENT).all() and (cnt == ISENT).all() and (pt == SENT).all()
    assert (scr == -1).all()
    with pytest.raises(_lib.AfmError, match="L must be in 1..8"):
        run("afm_screen_turnover_summary_f64", ac, cnt, pt, T, 2, 9, torch.empty(1, **opt))
    run("afm_screen_turnover_f64", *good[:9], 0, *good[10:])  # nd == 0: nothing to do
    torch.cuda.synchronize()
    assert (ac == SENT).all()


# ---- summary ---------------------------------------------------------------------------------------
def test_summary_bits_and_an_all_nan_series():
    import torch
    x, rows_idx, nrows, ref = small()
    ac, cnt, pt = (np.array(a) for a in ref)
    ac[:, 1, 2] = np.nan                                     # a series without a date
    nd, K, L = ac.shape
    st = torch.full((K * L * 4 * 2 + 3,), SENT, dtype=torch.float64, device="cuda:0")
    run("afm_screen_turnover_summary_f64", dev(ac), dev(cnt), dev(pt), nd, K, L, st)
    st = st.cpu().numpy()
    assert (st[K * L * 8:] == SENT).all()
    got = st[:K * L * 8].reshape(K, L, 4, 2)
    assert same(got, R.summary(ac, cnt, pt))
    assert got[1, 2, 0, 0] == 0 and np.isnan(got[1, 2, 0, 1])
    assert np.isnan(got[2, :, 0, 1]).all() and (got[0, 0, :, 0] > 0).all()
    st = torch.full((K * L * 8,), SENT, dtype=torch.float64, device="cuda:0")
    run("afm_screen_turnover_summary_f64", None, None, None, 0, K, L, st)    # no dates
    st = st.cpu().numpy().reshape(K, L, 4, 2)
    assert (st[..., 0] == 0).all() and np.isnan(st[..., 1]).all()
