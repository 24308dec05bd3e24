"""The signal-evaluation kernels of csrc/analyzer.hip called directly on hand-built grids, each
against the reference's own pandas / numpy statement on the same rows (tests/analyzer_ref.py,
pinned on the CPU by tests/test_analyzer_ref.py).  Bit for bit, NaN equal to NaN; no tolerance."""
import numpy as np
import pytest

import analyzer_ref as R
from helpers import same

pytestmark = pytest.mark.gpu

SENT = R.SENTINEL


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device=torch.device("cuda", 0))


def run(name, *args):
    from afm import _lib
    return _lib.run(name, *args)


# ---- afm_fwd_returns_f64 -------------------------------------------------------------------------
def test_fwd_returns_presence_word_edges():
    """T = 197 (no multiple of 4 or 64): day 63 of a word, an empty word between two present days,
    the k-th next day past the end, a never-present asset, a return of exactly 1 (kept) and the
    smallest one above it (NaN); every one of the 3 * T * lda cells, absent cells NaN."""
    import torch
    close, present = R.fwd_inputs()
    T, lda = close.shape
    fr = full((3, T, lda), SENT, torch.float64)
    run("afm_fwd_returns_f64", T, lda, dev(close), dev(R.pack_bits(present)), fr)
    assert same(fr.cpu().numpy(), R.fwd_returns_ref(close, present))


# ---- afm_xs_prepare_f64 / afm_xs_prepare_range_f64 -------------------------------------------------
def _prepare_buffers(T, lda):
    import torch
    return (full((4, T, lda), SENT, torch.float64), full((T, lda), -3, torch.int32),
            full((T,), -5, torch.int32))


@pytest.mark.parametrize("A,lda", [(32768, 32768), (20001, 20032), (70, 128), (3, 64)])
def test_prepare_cascade_and_buffered_means(A, lda):
    """The merge/dropna cascade with three different step masks and the per-date means over each
    step's own rows, with 0, 1, 7, 8, 127, 128, 129, 8191, 8192, 8193, 16385 and A surviving rows
    (capped at A): past 8192 rows the mean is numpy's buffered reduction, which on these inputs
    differs from one pairwise tree (test_prepare_inputs_tell_buffered_reduce_from_one_tree), so a
    kernel summing one tree fails here.  A = 32768 is the limit of the entry point; 20001 leaves a
    partial last word.  Then the range call on [5, 9): those dates bit-equal to the full call, all
    others untouched; and an empty range writes nothing."""
    import torch
    sig, fr = R.prepare_inputs(A, lda)
    T = sig.shape[0]
    ref = R.prepare_ref(sig[:, :A], fr[:, :, :A])
    sig_d, fr_d = dev(sig), dev(fr)
    scratch = torch.empty((T, lda), dtype=torch.float64, device=sig_d.device)
    rows, idx, nrows = _prepare_buffers(T, lda)
    run("afm_xs_prepare_f64", T, A, lda, sig_d, fr_d, scratch, rows, idx, nrows)
    rows, idx, nrows = rows.cpu().numpy(), idx.cpu().numpy(), nrows.cpu().numpy()
    assert same(nrows, [len(i) for i, _ in ref])
    for t, (ridx, rrows) in enumerate(ref):
        n = len(ridx)
        assert same(idx[t, :n], ridx), t
        assert same(rows[:, t, :n], rrows), t

    rows2, idx2, nrows2 = _prepare_buffers(T, lda)
    run("afm_xs_prepare_range_f64", T, A, lda, 7, 7, sig_d, fr_d, scratch, rows2, idx2, nrows2)
    assert (rows2 == SENT).all() and (idx2 == -3).all() and (nrows2 == -5).all()
    run("afm_xs_prepare_range_f64", T, A, lda, 5, 9, sig_d, fr_d, scratch, rows2, idx2, nrows2)
    rows2, idx2, nrows2 = rows2.cpu().numpy(), idx2.cpu().numpy(), nrows2.cpu().numpy()
    for t in range(T):
        if 5 <= t < 9:
            n = nrows[t]
            assert nrows2[t] == n and same(idx2[t, :n], idx[t, :n]), t
            assert same(rows2[:, t, :n], rows[:, t, :n]), t
        else:
            assert nrows2[t] == -5 and (idx2[t] == -3).all() and (rows2[:, t] == SENT).all(), t


def test_prepare_rejects_more_than_32768_assets():
    import torch
    from afm._lib import AfmError
    A, lda, T = 32769, 32832, 1
    sig = full((T, lda), 1.0, torch.float64)
    fr = full((3, T, lda), 1.0, torch.float64)
    rows, idx, nrows = _prepare_buffers(T, lda)
    with pytest.raises(AfmError, match=r"\(-1\)"):                      # AFM_E_ARG
        run("afm_xs_prepare_f64", T, A, lda, sig, fr, torch.empty_like(sig), rows, idx, nrows)
    torch.cuda.synchronize()
    assert (rows == SENT).all() and (idx == -3).all() and (nrows == -5).all()   # no launch


# ---- afm_xs_rank_f64 -----------------------------------------------------------------------------
RANK_COUNTS = {4160: [0, 1, 2, 2047, 2048, 2049, 4096, 4097, 4160],
               12352: [12288, 12289, 12352]}        # 12289, 12352: the search in global memory


@pytest.mark.parametrize("kind", ["normal", "ties", "zeros", "inf"])
@pytest.mark.parametrize("lda", [4160, 12352])
def test_rank_against_stable_argsort(lda, kind):
    """Exact ranks against a stable sort: around the 2048-row chunk of the LDS sort, several
    chunks, and dates too long for the LDS search; with heavy ties and all-equal dates (ties by
    row position), -0.0 tying with 0.0, and +-inf."""
    import torch
    counts = np.array(RANK_COUNTS[lda], dtype=np.int32)
    T = len(counts)
    v = R.rank_values(np.random.default_rng(lda + len(kind)), kind, (T, lda))
    rows = dev(v)
    skey = torch.empty((T, lda), dtype=torch.int64, device=rows.device)
    sidx = torch.empty((T, lda), dtype=torch.int32, device=rows.device)
    ra, rd = full((T, lda), -1, torch.int32), full((T, lda), -1, torch.int32)
    run("afm_xs_rank_f64", T, lda, rows, dev(counts), skey, sidx, ra, rd)
    ra, rd = ra.cpu().numpy(), rd.cpu().numpy()
    for t, n in enumerate(counts):
        wa, wd = R.rank_ref(v[t, :n])
        assert same(np.sort(ra[t, :n]), np.arange(1, n + 1)), t
        assert same(np.sort(rd[t, :n]), np.arange(1, n + 1)), t
        assert same(ra[t, :n], wa) and same(rd[t, :n], wd), t


# ---- afm_xs_stats_f64 ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["finite", "inf", "const", "retinf"])
def test_stats_against_pandas(kind):
    """IC, decile layer means and counts, and the factor-weighted top-10 returns per date against
    DataFrame.corr, groupby('layer').mean and the pivot statements; 1, 2, 9, 10, 11, 511, 512, 513,
    1025 and 1537 rows (the 512-row LDS chunks), as pivots of 10, 9 and 2 columns; ranks from
    afm_xs_rank_f64 and again from afm_xs_layers_f64, whose outputs must be identical.

    Non-finite rows: pandas 2.3.3's nancorr takes a row only if both values are finite
    (np.isfinite mask), so a +-inf factor or return row is skipped -- the kernel's skipping
    Welford path, entered in the first, a middle and the last chunk, with all-finite chunks after
    it; one finite row of two, or a constant factor, gives NaN.  group_mean resets a NaN Kahan
    compensation to 0, so a layer holding inf has mean inf (inf and -inf: NaN)."""
    import torch
    rows_h, counts = R.stats_inputs(kind)
    _, T, lda = rows_h.shape
    rows, nrows = dev(rows_h), dev(counts)
    ranks = []
    for fn in ("afm_xs_rank_f64", "afm_xs_layers_f64"):
        skey = torch.empty((T, lda), dtype=torch.int64, device=rows.device)
        sidx = torch.empty((T, lda), dtype=torch.int32, device=rows.device)
        ra, rd = full((T, lda), -1, torch.int32), full((T, lda), -1, torch.int32)
        run(fn, T, lda, rows, nrows, skey, sidx, ra, rd)
        ranks.append((ra, rd))
    for mcols in (10, 9, 2):
        sel = np.flatnonzero((counts <= mcols) | (mcols == 10)).astype(np.int32)
        nd = len(sel)
        assert counts[sel].max() == (1537 if mcols == 10 else mcols)
        want = R.stats_pandas([rows_h[:, t, :counts[t]] for t in sel])
        got = []
        for ra, rd in ranks:
            ic = full((nd, 3), SENT, torch.float64)
            lm = full((nd, 3, 10), SENT, torch.float64)
            lc = full((nd, 10), -1, torch.int32)
            port = full((nd, 3), SENT, torch.float64)
            run("afm_xs_stats_f64", T, lda, dev(sel), nd, rows, nrows, ra, rd, mcols, ic, lm, lc,
                port)
            got.append([x.cpu().numpy() for x in (ic, lm, lc, port)])
        for name, a, b, w in zip(("ic", "layer_mean", "layer_cnt", "port"), got[0], got[1], want):
            assert same(a, b), (mcols, name, "rank vs layers")
            assert same(a, w), (mcols, name, np.argwhere(~((a == w) | ((a != a) & (w != w)))))


# ---- afm_xs_series_f64 ---------------------------------------------------------------------------
def _series(lm, port, ic, year, nyears, year0):
    import torch
    nd = len(year)
    cum = full((nd, 3, 10), SENT, torch.float64)
    ls = full((nd, 3, 5), SENT, torch.float64)
    cp = full((nd, 3), SENT, torch.float64)
    ir = full((nyears, 3), SENT, torch.float64)
    scr = torch.empty((3 * nyears, nd), dtype=torch.float64, device=cum.device)
    run("afm_xs_series_f64", nd, dev(lm), dev(port), dev(ic), dev(year), nyears, year0, cum, ls,
        cp, ir, scr)
    return [x.cpu().numpy() for x in (cum, ls, cp, ir)]


NAMES = ("cum_layer", "ls", "cum_port", "ir")


def _years(nd):
    """nd dates over 2001..2017: 2002 has one date, 2003 none, the rest share what is left."""
    if nd < 4:
        return np.full(nd, 2001)
    rest = [y for y in range(2001, 2018) if y not in (2002, 2003)]
    y = np.sort(np.r_[2002, np.resize(rest, nd - 1)])
    return y


@pytest.mark.parametrize("nd", [1, 15, 16, 17, 403])
def test_series_against_pandas(nd):
    """Cumulative layers, long-short and top-10 series and the per-year IR against DataFrame.cumsum
    and groupby(year) mean() / std(): date counts around the 16-date load batches; a year without
    dates (IR NaN), a year with one sample (IR NaN), scattered NaN ICs and one (year, type) with
    NaNs only; NaN layer means (NaN on that date, the running sum carries on).  17 years keep the
    IC samples in LDS, 18 (one more, empty) in scratch: identical outputs."""
    year = _years(nd)
    lm, port, ic, year = R.series_inputs(year, seed=31 + nd)
    ic[year == 2005, 1] = np.nan
    want = R.series_pandas(lm, port, ic, year, 17, 2001)
    got17 = _series(lm, port, ic, year, 17, 2001)
    got18 = _series(lm, port, ic, year, 18, 2001)
    for name, a, b, w in zip(NAMES, got17, got18, want):
        assert same(a, w), name
        assert same(b[:len(a)], a), name
    assert np.isnan(got18[3][17]).all()
    if nd == 403:
        assert np.isnan(want[3][[1, 2]]).all() and np.isnan(want[3][4, 1])
        assert np.isfinite(want[3][[0, 3, 5, 16]]).all()
        assert np.isnan(want[0]).any()


@pytest.mark.parametrize("per_year", [(500, 20, 20), (20, 500, 20), (20, 20, 400)],
                         ids=["first", "middle", "last"])
def test_series_year_longer_than_lds_row(per_year):
    """A year with more evaluated dates than the 366 samples its LDS row holds (minute bars give
    thousands): the IR of that year and of every other year against pandas."""
    year = np.repeat(np.arange(2010, 2013), per_year)
    lm, port, ic, year = R.series_inputs(year, seed=sum(per_year), nan_frac=0.0)
    want = R.series_pandas(lm, port, ic, year, 3, 2010)
    got = _series(lm, port, ic, year, 3, 2010)
    assert np.isfinite(want[3]).all()
    for name, a, w in zip(NAMES, got, want):
        assert same(a, w), name
