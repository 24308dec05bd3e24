"""afm_ic_weights_f64 and afm_combine_f64 (csrc/combine.hip) called directly on hand-built buffers,
every output buffer filled with a sentinel first (tests/combine_ref.py, pinned on the CPU by
tests/test_combine_ref.py).

Methods 0..2 of the weights and the whole composite: bit for bit the float64 restatement, NaN
patterns included.  Method 3 (no stated order), per solved row, with A, m from the long-double
restatement and raw = w * info[2]:
  backward  eta = |A raw - m|_inf / (|A|_inf |raw|_inf + |m|_inf) <= (n_dates + 3 n_active) 2^-53,
            the first-order bound of a Gram accumulation followed by a Cholesky solve;
  forward   |raw - raw_ld|_inf / |raw_ld|_inf <= 2 cond_inf(A) * that bound;
and the active sets and n_dates are the reference's exactly.  A method-3 case counts only if the
reference alone solves at least half of its positions, which is asserted before the GPU is
touched: so min_periods = window goes with the clean input at window = 5 only, 10 % NaN per cell
with K <= 17 at window = 20, and whole NaN dates elsewhere (per cell the complete-date set D
empties).  The structural inputs (an all-NaN column, a constant column, a copy) need K >= 2.

The largest eta_engine / eta_float64 per case is printed (eta_float64: the float64 restatement of
the same row).  Measured on MI355X: see test_maxir_backward_and_forward_error."""
import functools

import numpy as np
import pytest

import combine_ref as R
from helpers import same

pytestmark = pytest.mark.gpu

SENT = -7.25
ND = 40
KS = [1, 3, 17, 65, 128]
KINDS = ["clean", "nan", "allnan", "const", "copy"]


def dev(x):
    import torch
    return torch.from_numpy(np.array(x)).to(torch.device("cuda", 0))     # (a writable copy)


def run(name, *args):
    from afm import _lib
    return _lib.run(name, *args)


@functools.lru_cache(maxsize=None)
def ic_input(kind, K, whole_dates=False, nd=ND):
    rng = np.random.default_rng(1000 * KINDS.index(kind) + K)
    ic = 0.02 + 0.05 * rng.standard_normal((nd, K, 3))
    if kind == "nan":
        if whole_dates:
            ic[rng.random(nd) < 0.1] = np.nan
        else:
            ic[rng.random(ic.shape) < 0.1] = np.nan
    elif kind == "allnan":
        ic[:, K // 2] = np.nan
    elif kind == "const":
        ic[:, K // 2] = 0.25                               # sums and their mean are exact: s = 0
    elif kind == "copy":
        ic[:, K - 1] = ic[:, 0]
    ic.setflags(write=False)
    return ic


def weights(ic, q, method, window, embargo, minp, shrink=0.5, nd=None):
    """The call -> (w [nd][K], info [nd][3]); one sentinel row behind each."""
    import torch
    nd = len(ic) if nd is None else nd
    K = ic.shape[1]
    w = torch.full((nd + 1, K), SENT, dtype=torch.float64, device="cuda:0")
    info = torch.full((nd + 1, 3), SENT, dtype=torch.float64, device="cuda:0")
    run("afm_ic_weights_f64", dev(ic), nd, K, q, method, window, embargo, minp, shrink, w, info)
    w, info = w.cpu().numpy(), info.cpu().numpy()
    assert (w[nd:] == SENT).all() and (info[nd:] == SENT).all()
    return w[:nd], info[:nd]


def roll_cases(method):
    """(window, embargo, min_periods, q, kind): every window x embargo x min_periods, q and the
    input walking with them so that each value of each meets each window."""
    out = []
    windows = ([1] if method == R.IC else []) + [5, 20]
    n = 0
    for window in windows:
        for embargo in (0, 1, 5):
            for minp in sorted({1 if method < R.ICIR else 2, window}):
                if method >= R.ICIR and minp < 2:
                    continue
                for kind in KINDS:
                    out.append((window, embargo, minp, (0, 2)[n % 2], kind))
                    n += 1
    return out


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("method", [R.EQUAL, R.IC, R.ICIR])
def test_rolling_weights_equal_the_restatement_bit_for_bit(method, K):
    for window, embargo, minp, q, kind in roll_cases(method):
        ic = ic_input(kind, K)
        what = (method, K, window, embargo, minp, q, kind)
        w, info = weights(ic, q, method, window, embargo, minp)
        rw, rinfo = R.ic_weights_ref(ic, q, method, window, embargo, minp)
        assert same(w, rw), what
        assert same(info, rinfo), what
        if method == R.EQUAL:
            assert (w == 1.0 / K).all() and (info == [K, 0, K]).all(), what
        else:
            assert np.isnan(w[:embargo]).all(), what       # nothing is known yet
            if kind == "clean" and minp <= 5:
                assert np.isfinite(w[embargo + minp - 1:]).all(), what


def maxir_cases(K, windows=(5, 20), embargos=(0, 1, 5)):
    out = []
    n = 0
    for window in windows:
        for embargo in embargos:
            for kind in KINDS:
                if K == 1 and kind in ("allnan", "const", "copy"):
                    continue
                minp = window if (kind == "clean" and window == 5) else 2
                whole = not (K <= 17 and window == 20)
                out.append((window, embargo, minp, (0, 2)[(n + embargo) % 2], kind, whole,
                            (0.1, 0.5, 1.0)[(n + window) % 3]))
                n += 1
    return out


@pytest.mark.parametrize("embargo", [0, 1, 5])
@pytest.mark.parametrize("window", [5, 20])
@pytest.mark.parametrize("K", KS)
def test_maxir_backward_and_forward_error(K, window, embargo):
    """Measured on MI355X over the cases of each K, the largest eta / bound: K = 1: 0.30, 3: 0.13,
    17: 0.031, 65: 0.009, 128: 0.003.  The largest eta_engine / eta_float64 of a single row: K =
    1: 44, 3: 18, 17: 3.2, 65: 3.2, 128: 2.4 -- the large ratios are rows on which the float64
    restatement happens to be nearly exact (K = 1: one division), not rows on which the engine is
    far off.  The other way round the plain float64 restatement misses the bound by up to 133 x at
    K = 1: a window mean that nearly cancels carries the rounding of its terms, and eta is measured
    against |m|.  The kernel therefore takes the mean by a compensated sum."""
    cases = maxir_cases(K, (window,), (embargo,))
    refs = []
    for window, embargo, minp, q, kind, whole, shrink in cases:   # the cap, before the GPU
        ic = ic_input(kind, K, whole)
        sys_ld, sys_64 = [], []
        wl, il = R.ic_weights_ref(ic, q, R.MAXIR, window, embargo, minp, shrink,
                                  dtype=np.longdouble, systems=sys_ld)
        R.ic_weights_ref(ic, q, R.MAXIR, window, embargo, minp, shrink, systems=sys_64)
        solved = int(np.isfinite(np.asarray(wl, dtype=np.float64)).all(axis=1).sum())
        assert solved >= ND // 2, (K, window, embargo, minp, kind, solved)
        refs.append((wl, il, sys_ld, sys_64))
    worst_ratio, worst_share = 0.0, 0.0
    for (window, embargo, minp, q, kind, whole, shrink), (wl, il, sys_ld, sys_64) in zip(cases,
                                                                                       refs):
        ic = ic_input(kind, K, whole)
        what = (K, window, embargo, minp, q, kind, shrink)
        w, info = weights(ic, q, R.MAXIR, window, embargo, minp, shrink)
        il64 = np.asarray(il, dtype=np.float64)
        assert same(info[:, :2], il64[:, :2]), what        # n_active, n_dates
        none = ~np.isfinite(il64[:, 2]) | (il64[:, 0] == 0)
        assert (np.isnan(w).all(axis=1) == none).all(), what
        for (i, a, D, A, m, xl), (_, _, _, _, _, x64) in zip(sys_ld, sys_64):
            if not len(a) or xl is None:
                assert np.isnan(w[i]).all(), (what, i)
                continue
            off = np.setdiff1d(np.arange(K), a)
            assert (w[i, off] == 0).all() and np.isfinite(w[i]).all(), (what, i)
            raw = (w[i, a] * info[i, 2]).astype(np.longdouble)
            ninf = lambda v: np.abs(v).max()                              # noqa: E731
            nA = np.abs(A).sum(axis=1).max()
            eta = float(ninf(A @ raw - m) / (nA * ninf(raw) + ninf(m)))
            e64 = x64.astype(np.longdouble)
            eta64 = float(ninf(A @ e64 - m) / (nA * ninf(e64) + ninf(m)))
            bound = (len(D) + 3 * len(a)) * R.U
            cond = np.linalg.cond(np.asarray(A, dtype=np.float64), np.inf)
            fwd = float(ninf(raw - xl) / ninf(xl))
            if eta64 > 0:
                worst_ratio = max(worst_ratio, eta / eta64)
            worst_share = max(worst_share, eta / bound)
            assert eta <= bound, (what, i, eta, bound)
            assert fwd <= 2 * cond * bound, (what, i, fwd, cond, bound)
    print(f"maxir K={K} window={window} embargo={embargo}: largest eta_engine / eta_float64 "
          f"{worst_ratio:.2f}, largest eta / bound {worst_share:.3f}")


@pytest.mark.parametrize("method", [R.EQUAL, R.IC, R.ICIR, R.MAXIR])
def test_no_look_ahead_and_truncation(method):
    rng = np.random.default_rng(5)
    for K, window, embargo, i0 in ((17, 5, 1, 20), (65, 20, 5, 30), (3, 20, 0, 12)):
        ic = np.array(ic_input("nan", K, True))
        minp, q = 2, 2
        w, info = weights(ic, q, method, window, embargo, minp)
        ic2 = ic.copy()
        tail = ic2[i0 - embargo + 1:]
        tail[...] = rng.standard_normal(tail.shape)
        tail[rng.random(tail.shape) < 0.3] = np.nan
        w2, info2 = weights(ic2, q, method, window, embargo, minp)
        assert same(w2[:i0 + 1], w[:i0 + 1]) and same(info2[:i0 + 1], info[:i0 + 1])
        if method != R.EQUAL:
            assert not same(w2, w)
        w3, info3 = weights(ic, q, method, window, embargo, minp, nd=25)
        assert same(w3, w[:25]) and same(info3, info[:25])


def test_maxir_row_is_a_function_of_its_window():
    """The same window at another position, other contents outside it: the same bits."""
    K, window, embargo, q = 65, 20, 1, 0
    ic = np.array(ic_input("clean", K))
    w, info = weights(ic, q, R.MAXIR, window, embargo, 2, 0.25)
    i = 30                                                  # its window: 10..29
    ic2 = np.full((ND, K, 3), np.nan)
    ic2[3:23] = ic[10:30]
    ic2[:3] = 9.0
    ic2[23:] = -3.0
    w2, info2 = weights(ic2, q, R.MAXIR, window, embargo, 2, 0.25)
    assert same(w2[23], w[i]) and same(info2[23], info[i]) and np.isfinite(w[i]).all()


def test_weights_argument_errors_write_nothing():
    import torch
    from afm._lib import AfmError
    ic = dev(ic_input("clean", 3))
    big = dev(np.zeros((4, 129, 3)))
    good = dict(nd=ND, K=3, q=0, method=R.ICIR, window=5, embargo=1, minp=2, shrink=0.5)
    bad = [dict(K=0), dict(K=129), dict(window=0), dict(window=1025), dict(embargo=-1),
           dict(minp=0), dict(minp=6), dict(method=R.ICIR, minp=1), dict(method=R.MAXIR, minp=1),
           dict(q=-1), dict(q=3), dict(method=4), dict(method=-1),
           dict(method=R.MAXIR, shrink=0.0), dict(method=R.MAXIR, shrink=1.5),
           dict(method=R.MAXIR, shrink=float("nan")), dict(nd=-1)]
    for change in bad:
        a = dict(good, **change)
        w = torch.full((ND, 129), SENT, dtype=torch.float64, device="cuda:0")
        info = torch.full((ND, 3), SENT, dtype=torch.float64, device="cuda:0")
        with pytest.raises(AfmError, match="afm_ic_weights_f64"):
            run("afm_ic_weights_f64", big if a["K"] == 129 else ic, a["nd"], a["K"], a["q"],
                a["method"], a["window"], a["embargo"], a["minp"], a["shrink"], w, info)
        torch.cuda.synchronize()
        assert (w == SENT).all() and (info == SENT).all(), change
    w = torch.full((ND, 3), SENT, dtype=torch.float64, device="cuda:0")
    info = torch.full((ND, 3), SENT, dtype=torch.float64, device="cuda:0")
    run("afm_ic_weights_f64", ic, 0, 3, 0, R.ICIR, 5, 1, 2, 0.5, w, info)      # nd == 0: AFM_OK
    run("afm_ic_weights_f64", ic, ND, 3, 0, R.IC, 1024, 0, 1024, 7.0, w, info)  # shrink: method 3's
    assert (info.cpu().numpy()[:, 0] == 0).all() and np.isnan(w.cpu().numpy()).all()


# ---- the composite ----------------------------------------------------------------------------

NROWS = [0, 1, 63, 64, 65, 128]


@functools.lru_cache(maxsize=None)
def grid_case(lda, P, content, nrows=tuple(NROWS)):
    rng = np.random.default_rng(lda + 7 * P + 13 * len(content))
    T = len(nrows)
    base = rng.standard_normal((P, T, lda))
    if content == "holes":
        base[rng.random(base.shape) < 0.15] = np.nan
        base[rng.random(base.shape) < 0.03] = np.inf
        base[rng.random(base.shape) < 0.03] = -np.inf
    elif content == "allnan":
        base[(P - 1) // 2] = np.nan
    n = np.minimum(np.array(nrows, dtype=np.int32), lda)
    rows_idx = np.full((T, lda), -1, dtype=np.int32)
    for t in range(T):
        pick = rng.permutation(lda)[:n[t]]
        rows_idx[t, :n[t]] = pick if t == T - 2 else np.sort(pick)   # one date in no order
    zs = np.stack([rng.standard_normal((P, lda)), 0.5 + rng.random((P, lda))], axis=2)
    zs[0, 3] = (0.0, np.inf)                               # sd = 0: a z that is not finite
    return base, rows_idx, n, zs


def weight_sets(nd, K, seed):
    rng = np.random.default_rng(seed)
    mixed = rng.standard_normal((nd, K))
    zeros = mixed.copy()
    zeros[rng.random((nd, K)) < 0.4] = 0.0
    zeros[0, 0] = -0.0
    nanrow = mixed.copy()
    nanrow[nd // 2] = np.nan
    nanrow[0, K - 1] = np.inf
    return {"mixed": mixed, "zeros": zeros, "nanrow": nanrow, "static": mixed[0].copy()}


def combine(dbuf, cols, dates, w, T, lda, zs=None, zcols=None, with_cnt=True):
    import torch
    out = torch.full((T, lda), SENT, dtype=torch.float64, device="cuda:0")
    cnt = torch.full((T, lda), -7, dtype=torch.int32, device="cuda:0") if with_cnt else None
    K = len(cols)
    run("afm_combine_f64", dbuf["base"], T * lda, T, lda, dev(np.asarray(cols, np.int32)), K,
        dbuf["zs"] if zs else None, None if zcols is None else dev(np.asarray(zcols, np.int32)),
        dev(np.asarray(dates, np.int32)), len(dates), dbuf["rows_idx"], dbuf["nrows"], dev(w),
        0 if w.ndim == 1 else K, out, cnt)
    return out.cpu().numpy(), (cnt.cpu().numpy() if with_cnt else None)


@pytest.mark.parametrize("zs", [False, True])
@pytest.mark.parametrize("K", [1, 2, 65, 128])
@pytest.mark.parametrize("lda", [64, 128])
def test_composite_equals_the_restatement_bit_for_bit(lda, K, zs):
    T = len(NROWS)
    P = max(K, 2)
    sent_o, sent_c = np.full((T, lda), SENT), np.full((T, lda), -7, dtype=np.int32)
    for content in ("clean", "holes", "allnan", "repeat"):
        base, rows_idx, nrows, ztab = grid_case(lda, P, "holes" if content == "repeat" else content)
        dbuf = dict(base=dev(base), rows_idx=dev(rows_idx), nrows=dev(nrows), zs=dev(ztab))
        cols = list(range(K))
        if content == "repeat" and K > 1:
            cols[-1] = cols[0]
        zcols = None if K % 2 else [P - 1 - c for c in cols]
        for dates in ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [4, 1]):
            for name, w in weight_sets(len(dates), K, 3 + K).items():
                what = (lda, K, zs, content, dates, name)
                out, cnt = combine(dbuf, cols, dates, w, T, lda, zs, zcols if zs else None)
                ro, rc = R.combine_ref(base, cols, dates, rows_idx, nrows, w, sent_o, sent_c,
                                       zs=ztab if zs else None, zcols=zcols if zs else None)
                assert same(out, ro), what
                assert same(cnt, rc), what
                for t in set(range(T)) - set(dates):       # the sentinel on every other date
                    assert (out[t] == SENT).all() and (cnt[t] == -7).all(), what
                for t in dates:                            # NaN / 0 off the rows
                    off = np.setdiff1d(np.arange(lda), rows_idx[t, :nrows[t]])
                    assert np.isnan(out[t, off]).all() and (cnt[t, off] == 0).all(), what
        o2, _ = combine(dbuf, cols, [2, 5], weight_sets(2, K, 1)["mixed"], T, lda, zs,
                        with_cnt=False)                    # cnt may be NULL
        r2, _ = R.combine_ref(base, cols, [2, 5], rows_idx, nrows, weight_sets(2, K, 1)["mixed"],
                              sent_o, sent_c, zs=ztab if zs else None)
        assert same(o2, r2)


@pytest.mark.parametrize("zs", [False, True])
def test_composite_against_itself(zs):
    """A column subset with its weights is the full call with the other weights zeroed; one date
    alone is that date within the full call."""
    lda, K, T = 128, 65, len(NROWS)
    base, rows_idx, nrows, ztab = grid_case(lda, K, "holes")
    dbuf = dict(base=dev(base), rows_idx=dev(rows_idx), nrows=dev(nrows), zs=dev(ztab))
    dates = [5, 0, 2, 4, 3, 1]
    w = weight_sets(len(dates), K, 9)["mixed"]
    sub = [1, 7, 8, 40, 64]
    wz = np.zeros_like(w)
    wz[:, sub] = w[:, sub]
    zc = list(range(K))
    full, cf = combine(dbuf, list(range(K)), dates, wz, T, lda, zs, zc if zs else None)
    part, cp = combine(dbuf, sub, dates, np.ascontiguousarray(w[:, sub]), T, lda, zs,
                       sub if zs else None)
    assert same(full, part) and same(cf, cp) and np.isfinite(full).any()
    whole, cw = combine(dbuf, list(range(K)), dates, w, T, lda, zs)
    for i, t in enumerate(dates):
        one, c1 = combine(dbuf, list(range(K)), [t], w[i:i + 1], T, lda, zs)
        assert same(one[t], whole[t]) and same(c1[t], cw[t])
        assert (np.delete(one, t, axis=0) == SENT).all()


def test_composite_over_several_workgroups_per_date():
    """lda = 320: two row blocks per date, the second partial; 255 / 256 / 257 rows."""
    lda, K = 320, 17
    nrows = (0, 1, 255, 256, 257, 320)
    T = len(nrows)
    base, rows_idx, n, ztab = grid_case(lda, K, "holes", nrows)
    dbuf = dict(base=dev(base), rows_idx=dev(rows_idx), nrows=dev(n), zs=dev(ztab))
    sent_o, sent_c = np.full((T, lda), SENT), np.full((T, lda), -7, dtype=np.int32)
    for dates in ([0, 1, 2, 3, 4, 5], [4, 2]):
        for name, w in weight_sets(len(dates), K, 21).items():
            for zs in (False, True):
                out, cnt = combine(dbuf, list(range(K)), dates, w, T, lda, zs)
                ro, rc = R.combine_ref(base, list(range(K)), dates, rows_idx, n, w, sent_o, sent_c,
                                       zs=ztab if zs else None)
                assert same(out, ro) and same(cnt, rc), (dates, name, zs)


def test_composite_argument_errors_write_nothing():
    import torch
    from afm._lib import AfmError
    lda, K, T = 64, 2, len(NROWS)
    base, rows_idx, nrows, ztab = grid_case(lda, 2, "clean")
    b, ri, nr = dev(base), dev(rows_idx), dev(nrows)
    cols, dates, w = dev(np.arange(2, dtype=np.int32)), dev(np.arange(T, dtype=np.int32)), \
        dev(np.ones((T, 2)))
    out = torch.full((T, lda), SENT, dtype=torch.float64, device="cuda:0")
    many = dev(np.zeros(129, dtype=np.int32))
    for args in ((b, T * lda, T, lda, cols, 0, None, None, dates, T, ri, nr, w, 0, out, None),
                 (b, T * lda, T, lda, many, 129, None, None, dates, T, ri, nr, w, 0, out, None),
                 (b, T * lda, T, 63, cols, 2, None, None, dates, T, ri, nr, w, 2, out, None),
                 (b, T * lda, T, lda, cols, 2, None, None, dates, T, ri, nr, w, 1, out, None),
                 (b, T * lda, T, lda, cols, 2, None, cols, dates, T, ri, nr, w, 2, out, None),
                 (b, T * lda, T, lda, cols, 2, None, None, dates, T, ri, nr, w, 2, b[1], None)):
        with pytest.raises(AfmError, match="afm_combine_f64"):
            run("afm_combine_f64", *args)
    torch.cuda.synchronize()
    assert (out == SENT).all() and same(b.cpu().numpy(), base)
    run("afm_combine_f64", b, T * lda, T, lda, cols, 2, None, None, dates, 0, ri, nr, w, 2, out,
        None)                                              # nd == 0: AFM_OK, nothing written
    assert (out == SENT).all()
