"""The layer / long-short / top-k kernels of the factor screen (csrc/screen_layers.hip) called
directly on hand-built rows / rows_idx / nrows and planes, against the reference's own pandas
statements per column on the rows restricted to the column's non-NaN cells (tests/layers_ref.py,
pinned on the CPU by tests/test_layers_ref.py), and against the single-signal kernels they batch.
Bit for bit, NaN equal to NaN; no tolerance.  The pandas reference runs per (date, column), so the
cases evaluate the planes of screen_ref's 130 that hold the special cells plus ordinary ones
(layers_ref.COLUMNS), each reference computed once."""
import functools

import numpy as np
import pytest

import analyzer_ref as R
import layers_ref as L
import screen_ref as S
from helpers import same

pytestmark = pytest.mark.gpu

SENT = -7.25
ISENT = -7
LDA = S.LDA
COLS = list(L.COLUMNS)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def run(name, *args):
    from afm import _lib
    return _lib.run(name, *args)


def device_case(planes, rows, rows_idx, nrows, zs=None):
    return dict(planes=dev(planes), rows=dev(rows), rows_idx=dev(rows_idx), nrows=dev(nrows),
                zs=None if zs is None else dev(zs), T=planes.shape[1], lda=planes.shape[2])


@functools.lru_cache(maxsize=None)
def case(kind: str, z: bool):
    """(device inputs, host inputs, (layer_mean, layer_cnt, port) of COLS on every date), once."""
    counts = L.counts_edges()
    host = L.layer_inputs(counts, kind)
    zs = S.zs_table(host[0].shape[0]) if z else None
    ref = L.layers_ref(*host, COLS, zs=zs, zcols=COLS if z else None)
    for a in ref:
        a.setflags(write=False)
    return device_case(*host, zs), host, ref


def screen_layers(d, cols, dates=None, zcols=None, extra=2):
    """afm_screen_layers_f64 on the case's buffers -> layer_mean, layer_cnt, port with ``extra``
    sentinel rows past nd."""
    import torch
    T, lda = d["T"], d["lda"]
    dates = np.arange(T) if dates is None else np.asarray(dates)
    nd, K = len(dates), len(cols)
    opt = dict(dtype=torch.float64, device="cuda:0")
    lm = torch.full((nd + extra, K, 3, 10), SENT, **opt)
    lc = torch.full((nd + extra, K, 10), ISENT, dtype=torch.int32, device="cuda:0")
    port = torch.full((nd + extra, K, 3), SENT, **opt)
    scr = torch.empty(nd * K * 40 + K, **opt)
    run("afm_screen_layers_f64", d["planes"], T * lda, T, lda, dev(np.asarray(cols, np.int32)), K,
        d["zs"], None if zcols is None else dev(np.asarray(zcols, np.int32)),
        dev(dates.astype(np.int32)), nd, d["rows"], d["rows_idx"], d["nrows"], lm, lc, port, scr)
    return lm.cpu().numpy(), lc.cpu().numpy(), port.cpu().numpy()


def layer_series(lm, port):
    import torch
    nd, K = port.shape[:2]
    opt = dict(dtype=torch.float64, device="cuda:0")
    cum = torch.full((nd + 1, K, 3, 10), SENT, **opt)
    ls = torch.full((nd + 1, K, 3, 5), SENT, **opt)
    cp = torch.full((nd + 1, K, 3), SENT, **opt)
    run("afm_screen_layer_series_f64", nd, K, dev(lm), dev(port), cum, ls, cp)
    cum, ls, cp = cum.cpu().numpy(), ls.cpu().numpy(), cp.cpu().numpy()
    assert (cum[nd:] == SENT).all() and (ls[nd:] == SENT).all() and (cp[nd:] == SENT).all()
    return cum[:nd], ls[:nd], cp[:nd]


def check(got, ref, nd):
    for name, g, r in zip(("layer_mean", "layer_cnt", "port"), got, ref):
        assert same(g[:nd], r), name
    assert (got[0][nd:] == SENT).all() and (got[1][nd:] == ISENT).all()
    assert (got[2][nd:] == SENT).all()


@pytest.mark.parametrize("kind", ["finite", "inf", "retinf"])
def test_layers_chunk_edge_counts(kind):
    """0 .. lda rows per date: screen_ref's counts, 9 / 10 / 11 rows (fewer rows than layers,
    exactly ten, eleven) and both sides of one, two and three staging chunks (kSlChunk, from the
    kernel).  'finite': rounded planes (ties by position) and constant planes (every row tied:
    the layers are the position-ordered ones); 'inf': +-inf ranked, NaN in the first chunk only,
    in a later chunk only, in the last row, on every row of a date (n_k == 0); 'retinf': inf in
    the returns.  Then the series of the same outputs."""
    chunk = L.kernel_constant("kSlChunk")
    counts = L.counts_edges()
    assert {0, 1, 9, 10, 11, chunk - 1, chunk, chunk + 1, 2 * chunk, 3 * chunk + 1, LDA} <= set(counts)
    d, host, ref = case(kind, False)
    got = screen_layers(d, COLS)
    check(got, ref, len(counts))
    lm, lc, port = ref
    if kind == "finite":
        t = counts.index(513)
        k = COLS.index(5)                                  # constant: layers by position
        assert same(lc[t, k], np.bincount([min(int(r / 513 * 10), 9) for r in range(1, 514)],
                                          minlength=10))
    else:
        t, k = counts.index(513), COLS.index(128)
        assert (lc[t, k] == 0).all() and np.isnan(lm[t, k]).all() and np.isnan(port[t, k]).all()
        assert lc[counts.index(LDA), COLS.index(1)].sum() == LDA - 3
        assert lc[counts.index(64), COLS.index(2)].sum() == 63
    assert (lc[counts.index(0)] == 0).all() and np.isnan(port[counts.index(0)]).all()
    cum, ls, cp = layer_series(got[0][:len(counts)], got[2][:len(counts)])
    rc, rl, rp = L.series_ref(lm, port)
    assert same(cum, rc) and same(ls, rl) and same(cp, rp)


@pytest.mark.parametrize("kind", ["finite", "inf"])
def test_layers_z_on_the_fly(kind):
    """zs given: z = (x - mu) * (1 / sd) from the same table in numpy; the {0, 0} row gives z = 0
    on every row -> all tied -> position-ordered layers.  zcols maps the columns to their rows
    (with repeated columns); zcols = NULL is row k."""
    d, host, ref = case(kind, True)
    nd = d["T"]
    got = screen_layers(d, COLS, zcols=COLS)
    check(got, ref, nd)
    raw, _, rawref = case(kind, False)
    assert not same(ref[0], rawref[0])
    pick = [0, 6, 6, 3, 0]                                 # repeated columns, their own zs rows
    cols = [COLS[i] for i in pick]
    got = screen_layers(d, cols, zcols=cols, extra=0)
    for g, r in zip(got, ref):
        assert same(g, r[:, pick])
    # zcols = NULL: column k takes row k of the table
    dates = [4, 9, 17]
    ident = [0, 1, 2, 3]
    want = L.layers_ref(*host, ident, dates=dates, zs=S.zs_table(130))
    got = screen_layers(d, ident, dates=dates)
    check(got, want, len(dates))


def test_layers_date_list_and_untouched_memory():
    """The evaluated dates a strict subset out of order -- the pivot of a column has the ranks of
    these dates only (here fewer than ten) -- then a longer one; rows of the outputs past nd keep
    the sentinel; cells of the planes outside rows_idx, and rows past nrows, are poisoned with NaN
    and must not change anything."""
    d, host, ref = case("inf", False)
    planes, rows, rows_idx, nrows = host
    counts = list(L.counts_edges())
    small = [counts.index(c) for c in (9, 1, 0, 2)]        # at most 9 rows: a pivot of 9 columns
    cols = [129, 0, 2, 2, 64]
    for dates in (small, [counts.index(c) for c in (1537, 9, 513, 0, 11, 65)]):
        want = L.layers_ref(*host, cols, dates=dates)
        check(screen_layers(d, cols, dates), want, len(dates))
    pl = np.full_like(planes, np.nan)
    rw = np.full_like(rows, np.nan)
    for t, n in enumerate(nrows):
        pl[:, t, rows_idx[t, :n]] = planes[:, t, rows_idx[t, :n]]
        rw[:, t, :n] = rows[:, t, :n]
    ri = rows_idx.copy()
    for t, n in enumerate(nrows):
        ri[t, n:] = -(1 << 30)                             # an index that must never be used
    dp = device_case(pl, rw, ri, nrows)
    dates = [counts.index(c) for c in (1537, 9, 513, 0, 11, 65)]
    check(screen_layers(dp, cols, dates), L.layers_ref(*host, cols, dates=dates), len(dates))


def test_layers_signed_zeros():
    """-0.0 / 0.0 / +-1 values: -0.0 ties with 0.0, ties go by row position."""
    counts = (64, 65, 513, 11, 1025)
    planes, rows, rows_idx, nrows = S.screen_inputs(counts, "finite")
    planes[0] = R.rank_values(np.random.default_rng(9), "zeros", planes[0].shape)
    assert (np.signbit(planes[0]) & (planes[0] == 0)).any()
    want = L.layers_ref(planes, rows, rows_idx, nrows, [0, 1])
    d = device_case(planes, rows, rows_idx, nrows)
    check(screen_layers(d, [0, 1]), want, len(counts))


def test_layers_large_lda():
    """lda = 32768, two columns: every row, and the largest row count of each register select
    (kSlFewRows, kSlSelectRows: the kernel's instantiations) with the first one past it."""
    few, thr = L.kernel_constant("kSlFewRows"), L.kernel_constant("kSlSelectRows")
    lda = L.kernel_constant("kSlMaxRows")
    assert lda == 32768 and few < thr < lda
    counts = (lda, thr, thr + 1, few, few + 1)
    nd = len(counts)
    rng = np.random.default_rng(77)
    planes = rng.normal(size=(2, nd, lda))
    planes[0] = np.round(planes[0], 2)
    planes[1, :, ::977] = np.nan
    planes[1, :, 5::1201] = np.inf
    rows = rng.normal(size=(4, nd, lda)) * 0.02
    rows_idx = np.full((nd, lda), -1, dtype=np.int32)
    for t, n in enumerate(counts):
        rows_idx[t, :n] = np.arange(lda) if n == lda else np.r_[
            np.sort(rng.permutation(lda - 1)[:n - 1]), lda - 1]
    nrows = np.array(counts, dtype=np.int32)
    want = L.layers_ref(planes, rows, rows_idx, nrows, [0, 1])
    d = device_case(planes, rows, rows_idx, nrows)
    got = screen_layers(d, [0, 1])
    check(got, want, nd)
    assert got[1][0, 0].sum() == lda and got[1][2, 0].sum() == thr + 1
    assert got[1][3, 0].sum() == few and got[1][4, 0].sum() == few + 1


def test_layers_equal_the_single_signal_kernels():
    """NaN-free planes: layer_mean, layer_cnt, port, cum_layer, ls and cum_port are those of
    afm_xs_layers_f64 + afm_xs_stats_f64 + afm_xs_series_f64 on the same rows with the plane as
    the signal, bit for bit."""
    import torch
    d, host, _ = case("finite", False)
    planes, rows, rows_idx, nrows = host
    T = d["T"]
    dates = np.flatnonzero(nrows > 0).astype(np.int32)
    nd = len(dates)
    cols = [0, 5, 70, 1]
    lm, lc, port = (a[:nd] for a in screen_layers(d, cols, dates))
    cum, ls, cp = layer_series(lm, port)
    opt = dict(dtype=torch.float64, device="cuda:0")
    iopt = dict(dtype=torch.int32, device="cuda:0")
    for k, c in enumerate(cols):
        r4 = rows.copy()
        for t, n in enumerate(nrows):
            r4[0, t, :n] = planes[c, t, rows_idx[t, :n]]
        r4 = dev(r4)
        skey = torch.empty((T, LDA), dtype=torch.int64, device="cuda:0")
        sidx, ra, rd = (torch.empty((T, LDA), **iopt) for _ in range(3))
        run("afm_xs_layers_f64", T, LDA, r4, d["nrows"], skey, sidx, ra, rd)
        ic = torch.empty((nd, 3), **opt)
        lm1, lc1, p1 = torch.empty((nd, 3, 10), **opt), torch.empty((nd, 10), **iopt), \
            torch.empty((nd, 3), **opt)
        run("afm_xs_stats_f64", T, LDA, dev(dates), nd, r4, d["nrows"], ra, rd, 10, ic, lm1, lc1,
            p1)
        cum1, ls1, cp1 = torch.empty_like(lm1), torch.empty((nd, 3, 5), **opt), \
            torch.empty_like(p1)
        ir = torch.empty((1, 3), **opt)
        scr = torch.empty((3, nd), **opt)
        run("afm_xs_series_f64", nd, lm1, p1, ic, dev(np.full(nd, 2001, np.int32)), 1, 2001,
            cum1, ls1, cp1, ir, scr)
        for name, mine, one in (("layer_mean", lm[:, k], lm1), ("layer_cnt", lc[:, k], lc1),
                                ("port", port[:, k], p1), ("cum_layer", cum[:, k], cum1),
                                ("ls", ls[:, k], ls1), ("cum_port", cp[:, k], cp1)):
            assert same(mine, one.cpu().numpy()), (name, c)


@pytest.mark.parametrize("nd", [1, 2, 700])
def test_layer_series(nd):
    """K = 3 columns of analyzer_ref.series_inputs-style data with NaN layer means and NaN top-k
    returns (a leading one, a run, the last date) against series_pandas per column."""
    rng = np.random.default_rng(nd)
    years = np.full(nd, 2001)
    parts = [R.series_inputs(years, seed=31 + k, nan_frac=0.05 + 0.2 * k) for k in range(3)]
    lm = np.stack([p[0] for p in parts], axis=1)
    port = np.stack([p[1] for p in parts], axis=1)
    port[rng.random(port.shape) < 0.1] = np.nan
    port[0, 1] = np.nan
    port[-1, 2, 0] = np.nan
    lm[:, 2, 1, 4] = np.nan                                # a layer that never has rows
    if nd > 100:
        port[40:60, 0, 2] = np.nan
    cum, ls, cp = layer_series(lm, port)
    rc, rl, rp = L.series_ref(lm, port)
    assert same(cum, rc) and same(ls, rl) and same(cp, rp)
    assert np.isnan(cp[0, 1]).all() and np.isnan(cum[:, 2, 1, 4]).all()


def test_argument_errors():
    """Bad arguments return AFM_E_ARG with a message and launch nothing (the outputs keep the
    sentinel)."""
    import torch
    from afm import _lib
    d, _, _ = case("finite", False)
    T = d["T"]
    opt = dict(dtype=torch.float64, device="cuda:0")
    cols, dates = dev(np.arange(3, dtype=np.int32)), dev(np.arange(T, dtype=np.int32))
    lm = torch.full((T, 3, 3, 10), SENT, **opt)
    lc = torch.full((T, 3, 10), ISENT, dtype=torch.int32, device="cuda:0")
    port = torch.full((T, 3, 3), SENT, **opt)
    scr = torch.full((T * 3 * 40 + 3,), SENT, **opt)
    good = [d["planes"], T * LDA, T, LDA, cols, 3, None, None, dates, T, d["rows"], d["rows_idx"],
            d["nrows"], lm, lc, port, scr]

    def bad(i, v, msg, j=None, w=None):
        a = list(good)
        a[i] = v
        if j is not None:
            a[j] = w
        with pytest.raises(_lib.AfmError, match=msg) as e:
            run("afm_screen_layers_f64", *a)
        assert "(-1)" in str(e.value)                      # AFM_E_ARG
    bad(5, 0, "K must be at least 1")
    bad(3, LDA - 32, "bad shape")
    bad(3, 32768 + 64, "lda must be at most 32768")
    bad(9, 1 << 30, "nd \\* K must be below 2\\^31")
    bad(9, 1 << 40, "nd \\* K must be below 2\\^31")
    bad(9, -1, "nd is negative")
    bad(0, None, "null buffer")
    bad(13, None, "null buffer")
    bad(16, None, "null buffer")
    bad(7, cols, "zcols without zs")
    torch.cuda.synchronize()
    assert (lm == SENT).all() and (lc == ISENT).all() and (port == SENT).all()
    assert (scr == SENT).all()
    cum, ls, cp = torch.full_like(lm, SENT), torch.full((T, 3, 3, 5), SENT, **opt), \
        torch.full_like(port, SENT)
    sgood = [T, 3, lm, port, cum, ls, cp]

    def sbad(i, v, msg):
        a = list(sgood)
        a[i] = v
        with pytest.raises(_lib.AfmError, match=msg) as e:
            run("afm_screen_layer_series_f64", *a)
        assert "(-1)" in str(e.value)
    sbad(1, 0, "K must be at least 1")
    sbad(0, -1, "nd is negative")
    sbad(2, None, "null buffer")
    sbad(6, None, "null buffer")
    torch.cuda.synchronize()
    assert (cum == SENT).all() and (ls == SENT).all() and (cp == SENT).all()
    run("afm_screen_layers_f64", *good)                    # the well-formed calls pass
    run("afm_screen_layer_series_f64", *sgood)
    torch.cuda.synchronize()
    assert not (port == SENT).any() and not (cp == SENT).any()
