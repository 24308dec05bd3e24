"""The factor-screening kernels of csrc/screen.hip called directly on hand-built rows / rows_idx /
nrows and planes, against the reference's own pandas statement on the same rows
(tests/screen_ref.py, pinned on the CPU by tests/test_screen_ref.py).  Bit for bit, NaN equal to
NaN; no tolerance.  Each reference is computed once per input kind for all 130 planes; the column
lists of the cases select from it."""
import functools

import numpy as np
import pytest

import screen_ref as S
from helpers import same

pytestmark = pytest.mark.gpu

SENT = -7.25
LDA = S.LDA


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def run(name, *args):
    from afm import _lib
    return _lib.run(name, *args)


@functools.lru_cache(maxsize=None)
def case(counts_name: str, kind: str, z: bool):
    """(device inputs, host ic reference [T][130][3]) of one input kind, made once."""
    counts = S.COUNTS_A if counts_name == "A" else S.counts_chunk_edges()
    planes, rows, rows_idx, nrows = S.screen_inputs(counts, kind)
    zs = S.zs_table(planes.shape[0]) if z else None
    ref = S.screen_ref(planes, rows, rows_idx, nrows, zs)
    ref.setflags(write=False)
    d = dict(planes=dev(planes), rows=dev(rows), rows_idx=dev(rows_idx), nrows=dev(nrows),
             zs=dev(zs) if z else None, T=len(counts))
    return d, ref


def screen_ic(d, cols, dates=None, zcols=None, extra=2):
    """afm_screen_ic_f64 on the case's buffers -> ic [nd + extra][K][3] (the extra rows keep the
    sentinel when the kernel writes only its own)."""
    import torch
    T = d["T"]
    dates = np.arange(T) if dates is None else np.asarray(dates)
    K = len(cols)
    ic = torch.full((len(dates) + extra, K, 3), SENT, dtype=torch.float64, device="cuda:0")
    run("afm_screen_ic_f64", d["planes"], T * LDA, T, LDA, dev(np.asarray(cols, np.int32)), K,
        d["zs"], None if zcols is None else dev(np.asarray(zcols, np.int32)),
        dev(dates.astype(np.int32)), len(dates), d["rows"], d["rows_idx"], d["nrows"], ic)
    return ic.cpu().numpy()


def column_list(K: int):
    """K columns of the 130 planes: K = 130 every plane in order; below that the planes with the
    special cells first (3, 5, 64, 66, 70, 129, 7), then the rest."""
    first = [3, 5, 64, 66, 70, 129, 7]
    return (first + [p for p in range(130) if p not in first])[:K] if K < 130 else list(range(130))


# K: one lane, both sides of the wave (64 lanes per workgroup), a short second workgroup, three
# workgroups
@pytest.mark.parametrize("K", [1, 63, 64, 65, 97, 130])
@pytest.mark.parametrize("kind", ["finite", "inf", "retinf"])
def test_ic_row_counts_and_column_counts(kind, K):
    """0, 1, 2, 63, 64, 65, 511, 512, 513, 1025, 1537 and lda rows per date; finite inputs with
    ties and constant columns (NaN IC); +-inf / NaN in single factor columns, so that lanes of one
    wave skip different rows (first chunk only, a later chunk only, the last row); inf in one
    return column only (that chain's factor mean differs from the other two).  rows_idx has gaps
    and the last asset; the planes' other cells are finite and must not be read."""
    d, ref = case("A", kind, False)
    cols = column_list(K)
    got = screen_ic(d, cols)
    assert same(got[:-2], ref[:, cols, :])
    assert (got[-2:] == SENT).all()


@pytest.mark.parametrize("kind", ["finite", "inf"])
def test_ic_staging_chunk_edges(kind):
    """kScreenRows - 1, kScreenRows, kScreenRows + 1 rows (one chunk / two), the same around two
    and three chunks (the asset indices are read two chunks ahead), and around kScreenInv (the
    1 / row-number ring is refilled), from the kernel's own constants."""
    chunk, ring = S.kernel_constant("kScreenRows"), S.kernel_constant("kScreenInv")
    counts = S.counts_chunk_edges()
    assert {chunk - 1, chunk, chunk + 1, 2 * chunk + 1, ring - 1, ring, ring + 1} <= set(counts)
    d, ref = case("edges", kind, False)
    cols = column_list(97)
    assert same(screen_ic(d, cols, extra=0), ref[:, cols, :])


def test_ic_repeated_and_descending_columns_and_date_subset():
    """A column list with a repeated column and planes in descending order; the evaluated dates a
    subset in non-ascending order; ic rows past nd keep the sentinel."""
    d, ref = case("A", "inf", False)
    cols = [129, 70, 66, 66, 64, 5, 3, 3, 0]
    dates = [11, 3, 9, 0, 10, 6]
    got = screen_ic(d, cols, dates)
    assert same(got[:len(dates)], ref[dates][:, cols, :])
    assert (got[len(dates):] == SENT).all()


@pytest.mark.parametrize("kind", ["finite", "inf"])
def test_ic_z_on_the_fly(kind):
    """zs given: z = (x - mu) * (1 / sd) from the same table in numpy; the {0, 0} row gives z = 0
    -> constant -> NaN.  zcols maps the columns to their rows; zcols = NULL is row k."""
    d, ref = case("A", kind, True)
    cols = column_list(97)
    got = screen_ic(d, cols, zcols=cols, extra=0)
    assert same(got, ref[:, cols, :])
    assert np.isnan(got[:, cols.index(7), :]).all()
    ident = list(range(70))
    assert same(screen_ic(d, ident, extra=0), ref[:, ident, :])
    raw, _ = case("A", kind, False)
    assert not same(got, screen_ic(raw, cols, extra=0))


# ---- afm_screen_summary_f64 -----------------------------------------------------------------------
def test_summary_year_lengths():
    """Years of 1, 2, 366, 367 and 5,000 dates (minute bars), a year split in two runs by another
    year's dates, a year whose ICs are all NaN, a (k, q) with no IC at all and one with exactly
    one; against pandas mean / std per column, bit for bit."""
    import torch
    year = np.repeat([2000, 2001, 2002, 2003, 2004, 2005, 2003, 2006],
                     [1, 2, 366, 200, 5000, 40, 167, 30]).astype(np.int32)   # 2003: 367, split
    nd, K = len(year), 4
    rng = np.random.default_rng(71)
    ic = rng.uniform(-1, 1, (nd, K, 3))
    ic[rng.random(ic.shape) < 0.05] = np.nan
    ic[year == 2005] = np.nan                              # a year without ICs
    ic[:, 1, 0] = np.nan                                   # n = 0
    ic[:, 1, 1] = np.nan
    ic[777, 1, 1] = 0.25                                   # n = 1
    y0, ny = 2000, 7
    stats_ref, ir_ref = S.summary_pandas(ic, year, ny, y0)
    stats = torch.full((K, 3, 5), SENT, dtype=torch.float64, device="cuda:0")
    ir = torch.full((ny, K, 3), SENT, dtype=torch.float64, device="cuda:0")
    scr = torch.empty((K, 3, 2, nd), dtype=torch.float64, device="cuda:0")
    run("afm_screen_summary_f64", dev(ic), nd, K, dev(year), ny, y0, stats, ir, scr)
    stats, ir = stats.cpu().numpy(), ir.cpu().numpy()
    assert same(ir, ir_ref)
    assert same(stats, stats_ref)
    assert stats[1, 0, 0] == 0 and stats[1, 1, 0] == 1 and stats[1, 1, 1] == 0.25
    assert np.isnan(ir[5]).all() and np.isnan(ir[0]).all() and not np.isnan(ir[3, 0]).any()


# ---- argument errors ---------------------------------------------------------------------------------
def test_argument_errors():
    import torch
    from afm import _lib
    d, _ = case("A", "finite", False)
    T = d["T"]
    cols, dates = dev(np.arange(3, dtype=np.int32)), dev(np.arange(T, dtype=np.int32))
    ic = torch.empty((T, 3, 3), dtype=torch.float64, device="cuda:0")
    good = [d["planes"], T * LDA, T, LDA, cols, 3, None, None, dates, T, d["rows"], d["rows_idx"],
            d["nrows"], ic]

    def bad(i, v, msg):
        a = list(good)
        a[i] = v
        with pytest.raises(_lib.AfmError, match=msg) as e:
            run("afm_screen_ic_f64", *a)
        assert "(-1)" in str(e.value)                      # AFM_E_ARG
    bad(5, 0, "K must be at least 1")
    bad(3, LDA - 32, "bad shape")
    bad(0, None, "null buffer")
    bad(13, None, "null buffer")
    bad(7, cols, "zcols without zs")
    st = torch.empty((3, 3, 5), dtype=torch.float64, device="cuda:0")
    ir = torch.empty((2, 3, 3), dtype=torch.float64, device="cuda:0")
    scr = torch.empty((3, 3, 2, T), dtype=torch.float64, device="cuda:0")
    yr = dev(np.full(T, 2001, dtype=np.int32))
    sgood = [ic, T, 3, yr, 2, 2001, st, ir, scr]

    def sbad(i, v, msg):
        a = list(sgood)
        a[i] = v
        with pytest.raises(_lib.AfmError, match=msg) as e:
            run("afm_screen_summary_f64", *a)
        assert "(-1)" in str(e.value)
    sbad(2, 0, "K must be at least 1")
    sbad(4, 321, "nyears")
    sbad(4, -1, "nyears")
    sbad(8, None, "null buffer")
    run("afm_screen_summary_f64", *sgood)                  # the well-formed call passes
