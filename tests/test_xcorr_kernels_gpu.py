"""The cross-factor correlation kernels of csrc/xcorr.hip called directly on hand-built rows_idx /
nrows and planes (tests/xcorr_ref.py, pinned on the CPU by tests/test_xcorr_ref.py).

Against the extended-precision reference: equal NaN patterns and |xc - ref| <= 32 max(n, 64) 2^-53
of the date's row count n.  Bit for bit: an entry depends on its two columns' values on the date's
rows alone (K, the positions in cols, the other columns and dates, fast path or masked), the matrix
is symmetric, the diagonal is 1.0 or NaN; the summary against numpy.  The reference is computed
once for all 130 planes; the column lists of the cases select from it."""
import functools

import numpy as np
import pytest

import xcorr_ref as X
from helpers import same

pytestmark = pytest.mark.gpu

SENT = -7.25
LDA = X.LDA


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def run(name, *args):
    from afm import _lib
    return _lib.run(name, *args)


@functools.lru_cache(maxsize=None)
def case(z: bool = False):
    planes, rows_idx, nrows = X.xcorr_inputs()
    zs = X.zs_table(planes.shape[0]) if z else None
    d = dict(planes=dev(planes), rows_idx=dev(rows_idx), nrows=dev(nrows),
             zs=dev(zs) if z else None, T=len(nrows))
    return d, (planes, rows_idx, nrows, zs)


@functools.lru_cache(maxsize=None)
def ref_all():
    """xc [T][130][130] of the reference on the raw values, made once."""
    planes, rows_idx, nrows, _ = case()[1]
    ref = X.xcorr_ref(planes, rows_idx, nrows)
    ref.setflags(write=False)
    return ref


def xcorr(d, cols, dates=None, zcols=None, extra=2, rows=None):
    """afm_screen_xcorr_f64 on the case's buffers -> xc [nd + extra][K][K] (the extra rows keep
    the sentinel when the kernel writes only its own)."""
    import torch
    T = d["T"]
    dates = np.arange(T) if dates is None else np.asarray(dates)
    K = len(cols)
    xc = torch.full((len(dates) + extra, K, K), SENT, dtype=torch.float64, device="cuda:0")
    run("afm_screen_xcorr_f64", d["planes"], T * LDA, T, LDA, dev(np.asarray(cols, np.int32)), K,
        d["zs"], None if zcols is None else dev(np.asarray(zcols, np.int32)),
        dev(dates.astype(np.int32)), len(dates), rows, d["rows_idx"], d["nrows"], xc)
    return xc.cpu().numpy()


@functools.lru_cache(maxsize=None)
def got_all():
    g = xcorr(case()[0], list(range(130)), extra=0)
    g.setflags(write=False)
    return g


def check(got, ref, counts, what=""):
    """NaN patterns equal; every date within its bound; never beyond [-1, 1].  Prints the figures
    (largest error, bound) before it asserts."""
    assert got.shape == ref.shape
    worst = (0.0, 0, 1.0)
    for i, n in enumerate(counts):
        assert (np.isnan(got[i]) == np.isnan(ref[i])).all(), (what, int(n))
        if not np.isnan(ref[i]).all():
            err = float(np.nanmax(np.abs(got[i] - ref[i])))
            if err / X.tolerance(n) >= worst[0] / worst[2]:
                worst = (err, int(n), X.tolerance(n))
    print(f"xcorr error {what}: max |xc - ref| = {worst[0]:.3e} at n = {worst[1]} "
          f"(bound {worst[2]:.3e})")
    for i, n in enumerate(counts):
        if not np.isnan(ref[i]).all():
            assert np.nanmax(np.abs(got[i] - ref[i])) <= X.tolerance(n), (what, int(n))
    assert not (np.abs(got[~np.isnan(got)]) > 1.0).any()


SPECIAL = [X.OFFSET, X.NAN5[0], X.CONST, X.BIG, X.SMALL, 14, 15, 16, 17, X.TIES, X.NAN5[1],
           X.NAN5[2], X.ALLNAN, X.ONEROW, X.EVEN, X.ODD, X.INFS, X.CONSTNAN, X.OFFNAN, X.LAST]
HOLES = set(X.NAN5) | {X.ALLNAN, X.ONEROW, X.EVEN, X.ODD, X.INFS, X.CONSTNAN, X.OFFNAN, X.LAST}


def column_list(K: int, kind: str):
    """'mixed': K = 130 every plane in order (block 0 all finite: the fast path beside masked
    blocks); below that the special planes first, then the rest.  'finite': planes without a
    missing cell only, the special ones among them first -- every workgroup on the fast path."""
    if kind == "finite":
        first = [p for p in SPECIAL if p not in HOLES]
        return (first + [p for p in range(129) if p not in first and p not in HOLES])[:K]
    if K == 130:
        return list(range(130))
    return (SPECIAL + [p for p in range(130) if p not in SPECIAL])[:K]


# K: one column, two, both sides of the 16-column tile and of the 64-column block, two and three
# blocks (3 and 6 block pairs per date)
KS = [1, 2, 15, 16, 17, 64, 65, 97, 130]


# (all finite at K = 130 does not exist: 118 planes have no missing cell; the K = 130 list has its
# first block all finite)
@pytest.mark.parametrize("kind,K", [("finite", K) for K in KS[:-1]] + [("mixed", K) for K in KS])
def test_xcorr_row_counts_and_column_counts(kind, K):
    """0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 511, 513 and lda rows per date, and kXcRows - 1,
    kXcRows, kXcRows + 1 and 2 kXcRows + 1 (the staging chunk, from the kernel's constant).  All
    finite (the fast path): ties, heavy ties, a constant column (NaN row, column and diagonal), the
    1e6-offset column, columns scaled by 1e7 and 1e-9, two exactly collinear pairs (within the
    bound of +-1, never beyond).  Mixed: 5 % NaN, a column all NaN on one date, a column finite on
    one row, two columns with disjoint presence, +-inf cells, a constant column with NaN.
    rows_idx has gaps and the last asset; the planes' other cells are finite junk."""
    d, (planes, rows_idx, nrows, _) = case()
    c = X.kernel_constant("kXcRows")
    assert {0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 511, 513, LDA, c - 1, c + 1,
            2 * c + 1} <= set(nrows.tolist())
    cols = column_list(K, kind)
    assert len(cols) == K
    got = xcorr(d, cols)
    ref = ref_all()[:, cols][:, :, cols]
    check(got[:-2], ref, nrows, f"{kind} K={K}")
    assert (got[-2:] == SENT).all()
    if K >= 17:
        i5 = cols.index(X.CONST)
        assert np.isnan(got[:-2, i5, :]).all() and np.isnan(got[:-2, :, i5]).all()
        for a, b, sign in X.COLLINEAR:
            r = got[:-2, cols.index(a), cols.index(b)]
            big = nrows >= 2
            assert (np.abs(r[big] - sign) <= [X.tolerance(n) for n in nrows[big]]).all()
            assert (np.abs(r[big]) <= 1.0).all()
    if kind == "mixed" and K >= 64:
        assert np.isnan(got[:-2, cols.index(X.EVEN), cols.index(X.ODD)]).all()     # n = 0
        assert np.isnan(got[:-2, cols.index(X.ONEROW), :]).all()
        t = int(np.flatnonzero(nrows == X.ALLNAN_COUNT)[0])
        assert np.isnan(got[t, cols.index(X.ALLNAN), :]).all()
        assert np.isnan(got[:-2, cols.index(X.CONSTNAN), :]).all()


def test_xcorr_symmetry_and_diagonal():
    """Full and bitwise symmetric; the diagonal exactly 1.0 where the column has a variance on the
    date, else NaN."""
    got, ref = got_all(), ref_all()
    assert same(got, got.transpose(0, 2, 1))
    dg = np.diagonal(got, axis1=1, axis2=2)
    assert ((dg == 1.0) | np.isnan(dg)).all()
    assert (np.isnan(dg) == np.isnan(np.diagonal(ref, axis1=1, axis2=2))).all()
    assert (dg == 1.0).sum() > 0 and np.isnan(dg).sum() > 0


def test_xcorr_entry_depends_on_its_two_columns_only():
    """Bit for bit: a permuted column list with a repeat; K = 3 taken out of the K = 130 call; a
    date subset in non-ascending order (xc rows past nd keep the sentinel); a finite pair beside an
    all-finite neighbour (fast path) and beside a neighbour with NaN (masked)."""
    d, (_, _, nrows, _) = case()
    base = got_all()
    rng = np.random.default_rng(3)
    cols = [int(c) for c in rng.permutation(130)[:70]] + [X.OFFSET, X.NAN5[0]]
    cols += [cols[3], cols[3], X.NAN5[0]]                    # repeats: the same column twice
    got = xcorr(d, cols, extra=0)
    assert same(got, base[:, cols][:, :, cols])
    three = [X.OFFSET, X.NAN5[0], 100]
    assert same(xcorr(d, three, extra=0), base[:, three][:, :, three])
    dates = [14, 3, 13, 0, 17, 9, 9]
    sub = xcorr(d, three, dates)
    assert same(sub[:len(dates)], base[dates][:, three][:, :, three])
    assert (sub[len(dates):] == SENT).all()
    fast, masked = xcorr(d, [0, 1, 3], extra=0), xcorr(d, [0, 1, X.NAN5[0]], extra=0)
    assert same(fast[:, :2, :2], masked[:, :2, :2]) and same(fast[:, :2, :2], base[:, :2, :2])
    big = nrows >= 15
    assert np.isnan(masked[big, 2, :2]).sum() == 0 and not same(fast[big, 2], masked[big, 2])
    # the rows argument is not read: a tensor in its place changes nothing
    import torch
    junk = torch.full((4, d["T"], LDA), float("nan"), dtype=torch.float64, device="cuda:0")
    assert same(xcorr(d, three, extra=0, rows=junk), base[:, three][:, :, three])


def test_xcorr_z_on_the_fly():
    """zs given: z = (x - mu) * (1 / sd) from the same table in numpy; the {0, 0} row gives z = 0
    -> a constant column -> NaN.  zcols maps the columns to their rows; zcols = NULL is row k."""
    d, (planes, rows_idx, nrows, zs) = case(True)
    cols = X.Z_COLS
    ref = X.xcorr_ref(planes, rows_idx, nrows, cols, zs)
    got = xcorr(d, cols, zcols=cols, extra=0)
    check(got, ref, nrows, "z")
    i7 = cols.index(7)
    assert np.isnan(got[:, i7, :]).all() and np.isnan(got[:, :, i7]).all()
    ident = X.Z_IDENT
    check(xcorr(d, ident, extra=0),
          X.xcorr_ref(planes, rows_idx, nrows, ident, zs, np.arange(len(ident))), nrows,
          "z, zcols = NULL")
    # the same plane under two zs rows is not the same column; under the same row it is
    two = xcorr(d, [3, 3, 3], zcols=[3, 4, 3], extra=0)
    t = int(np.flatnonzero(nrows == 65)[0])
    assert two[t, 0, 2] == 1.0 and two[t, 0, 1] != 1.0 and abs(two[t, 0, 1]) < 1.0
    raw = xcorr(case()[0], cols, extra=0)
    assert not same(got, raw)


def summary(xc):
    import torch
    nd, K, _ = xc.shape
    st = torch.full((K, K, 3), SENT, dtype=torch.float64, device="cuda:0")
    run("afm_screen_xcorr_summary_f64", dev(xc), nd, K, st)
    return st.cpu().numpy()


def test_summary_bit_exact_on_the_kernels_output():
    """n, mean r and mean |r| of every pair over the dates against numpy on the xc just produced:
    pairs that are NaN on every date (the constant column), on some (the all-NaN date), on none."""
    xc = np.array(got_all())
    st = summary(xc)
    assert same(st, X.summary_ref(xc))
    assert st[X.CONST, 0, 0] == 0 and np.isnan(st[X.CONST, 0, 1:]).all()
    full = st[0, 1, 0]
    assert 0 < st[X.ALLNAN, 0, 0] < full and st[X.EVEN, X.ODD, 0] == 0
    assert st[0, 0, 1] == 1.0 and st[0, 0, 2] == 1.0


def test_summary_long_series_and_dates_in_the_order_given():
    """9,000 dates (past numpy's 8192-element reduction buffer), K = 3; a pair with no entry and
    one with a single entry; the order of the dates matters to the rounding and is kept."""
    rng = np.random.default_rng(5)
    xc = rng.uniform(-1, 1, (9000, 3, 3))
    xc[rng.random(xc.shape) < 0.1] = np.nan
    xc[:, 0, 1] = np.nan
    xc[:, 2, 2] = np.nan
    xc[17, 2, 2] = -0.5
    st = summary(xc)
    assert same(st, X.summary_ref(xc))
    assert st[0, 1, 0] == 0 and np.isnan(st[0, 1, 1]) and np.isnan(st[0, 1, 2])
    assert st[2, 2, 0] == 1 and st[2, 2, 1] == -0.5 and st[2, 2, 2] == 0.5
    assert same(summary(xc[::-1]), X.summary_ref(xc[::-1]))
    one = summary(xc[:1])
    assert same(one, X.summary_ref(xc[:1]))


def test_argument_errors():
    import torch
    from afm import _lib
    d, _ = case()
    T = d["T"]
    cols, dates = dev(np.arange(3, dtype=np.int32)), dev(np.arange(T, dtype=np.int32))
    xc = torch.empty((T, 3, 3), dtype=torch.float64, device="cuda:0")
    good = [d["planes"], T * LDA, T, LDA, cols, 3, None, None, dates, T, None, d["rows_idx"],
            d["nrows"], xc]

    def bad(i, v, msg):
        a = list(good)
        a[i] = v
        with pytest.raises(_lib.AfmError, match=msg) as e:
            run("afm_screen_xcorr_f64", *a)
        assert "(-1)" in str(e.value)                      # AFM_E_ARG
        assert "afm_screen_xcorr_f64" in str(e.value)
    bad(5, 0, "K must be at least 1")
    bad(3, LDA - 32, "bad shape")
    bad(0, None, "null buffer")
    bad(4, None, "null buffer")
    bad(8, None, "null buffer")
    bad(11, None, "null buffer")
    bad(12, None, "null buffer")
    bad(13, None, "null buffer")
    bad(7, cols, "zcols without zs")
    bad(9, -1, "nd is negative")
    bad(9, 1 << 31, "below 2\\^31")
    run("afm_screen_xcorr_f64", *good)                     # the well-formed call passes
    a = list(good)
    a[9] = 0
    run("afm_screen_xcorr_f64", *a)                        # no dates: nothing written
    st = torch.empty((3, 3, 3), dtype=torch.float64, device="cuda:0")
    sgood = [xc, T, 3, st]

    def sbad(i, v, msg):
        a = list(sgood)
        a[i] = v
        with pytest.raises(_lib.AfmError, match=msg) as e:
            run("afm_screen_xcorr_summary_f64", *a)
        assert "(-1)" in str(e.value)
    sbad(2, 0, "K must be at least 1")
    sbad(2, 1 << 16, "K \\* K")
    sbad(1, -1, "nd is negative")
    sbad(0, None, "null buffer")
    sbad(3, None, "null buffer")
    run("afm_screen_xcorr_summary_f64", *sgood)            # the well-formed call passes
    run("afm_screen_xcorr_summary_f64", None, 0, 3, st)    # no dates: n = 0, NaN means
    s0 = st.cpu().numpy()
    assert (s0[:, :, 0] == 0).all() and np.isnan(s0[:, :, 1:]).all()
