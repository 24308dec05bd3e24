"""The kernels of csrc/portfolio.hip called directly -- afm_rebalance_f64,
afm_min_variance_weights_f64, afm_pnl_scan_f64 and afm_bootstrap_pnl_f64 through _lib.run on
hand-built device tensors, no pandas and no PortfolioManager -- at the branch points random panels
do not reach, against the plain numpy reference of tests/portfolio_ref.py (pinned to
oracle/portfolio.py by tests/test_portfolio_ref.py, where every case's claimed property is
asserted too).

Every output is prefilled: -1 for the books, -7 for the other integers, a NaN payload no kernel
writes for the doubles, and "untouched past k" is asserted wherever the kernels are specified not
to write.  No tolerance is new: bit equality (helpers.same), or one of the three existing bars --
the Welford covariance bit for bit where holes are present (k <= 32), 1e-12 max|S| for the
one-pass MFMA covariance (k > 32), weights within 1e-9 with |sum w - 1| < 1e-12 and identical
bound sets."""
import numpy as np
import pytest

import portfolio_ref as R
from helpers import same

pytestmark = pytest.mark.gpu

SENT = 0x7FF8DEAD0000BEEF                  # the doubles' prefill: a NaN payload no kernel writes
ISENT = -7                                 # the integers' prefill (the books': -1)
KEYS = ("value", "turnover", "long_ret", "short_ret")


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sent(*shape):
    import torch
    return torch.full(shape, SENT, dtype=torch.int64, device="cuda").view(torch.float64)


def _ints(shape, dtype, fill=ISENT):
    import torch
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.int64) == np.int64(SENT)).all())


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in out.items()}


_DEV = {}


def _upload(pn):
    """a panel's device planes and bit words (uploaded once per panel)"""
    from afm.grid import pack_bits
    d = _DEV.get(id(pn))
    if d is None:
        hb = pn["hbits"] if "hbits" in pn else np.ones(pn["hist"].shape, dtype=bool)
        d = _DEV[id(pn)] = dict(pn=pn, pred=_cuda(pn["pred"]), hist=_cuda(pn["hist"]),
                                close=_cuda(pn["close"]), tmr=_cuda(pn["tmr"]),
                                tbits=pack_bits(_cuda(pn["trad"])), hbits=pack_bits(_cuda(hb)))
    return d


def _rebalance(d, dates, *, A, top_n, window=None, h_range=None, lo=0.0, hi=0.1):
    """afm_rebalance_f64 on prefilled outputs -> dict of numpy arrays"""
    import torch
    from afm import _lib
    T, lda = d["pred"].shape
    nd = len(dates)
    out = dict(k=_ints((nd,), torch.int32), books=_ints((nd, 2, R.MAX_BOOK), torch.int32, -1),
               weights=_sent(nd, 2, R.MAX_BOOK), sums=_sent(nd, 4),
               upos=_ints((nd, 2, 2, R.MAX_BOOK), torch.int32), usize=_ints((nd, 2), torch.int64),
               status=_ints((nd,), torch.int32))
    h0, h1 = h_range if h_range is not None else (0, T)
    _lib.run("afm_rebalance_f64", T, A, lda, _cuda(np.asarray(dates, dtype=np.int32)), nd,
             d["pred"], d["tbits"], d["hist"], d["hbits"], h0, h1,
             -1 if window is None else int(window), d["close"], d["tmr"], int(top_n), float(lo),
             float(hi), out["k"], out["books"], out["weights"], out["sums"], out["upos"],
             out["usize"], out["status"])
    return _host(out)


def _check_books(got, i, k, L, S, upos=None):
    """books and union positions of date i exact, everything past k untouched"""
    for side, bk in enumerate((L, S)):
        assert same(got["books"][i, side, :k], bk), (i, side)
        assert (got["books"][i, side, k:] == -1).all(), (i, side)
        assert _untouched(got["weights"][i, side, k:]), (i, side)
        assert (got["upos"][i, side, :, k:] == ISENT).all(), (i, side)
        if upos is not None:
            assert same(got["upos"][i, side, :, :k], upos[side]), (i, side)


# ---- (a) selection: rebalance_kernel phases 1-2, select_top_reg, digit_pick, select_top --------
@pytest.mark.parametrize("name", sorted(R.selection_cases()))
def test_selection(name):
    """Panels of 4 dates, all rebalanced, window = 2; k * hi <= 1, so the weights are exactly hi
    and the covariance plays no part.  k, books, weights, the four sums, upos and usize exact."""
    from oracle.xs import np_sum
    c = R.selection_cases()[name]
    e = R.expected_selection(c, np_sum)
    got = _rebalance(_upload(c), range(R.SEL_T), A=c["A"], top_n=c["top_n"], window=2,
                     hi=c["hi"])
    print(name, "k", got["k"].tolist(), "usize", got["usize"].tolist())
    assert same(got["k"], e["k"])
    assert (got["status"] == 0).all()
    for t in range(R.SEL_T):
        k = int(e["k"][t])
        L, S = e["books"][t]
        _check_books(got, t, k, L, S, e["upos"][t])
        for side in range(2):
            assert same(got["weights"][t, side, :k], np.full(k, c["hi"])), (t, side)
        assert same(got["sums"][t], np.array(e["sums"][t])), (t, got["sums"][t], e["sums"][t])
        assert same(got["usize"][t], np.array(e["usize"][t])), t


# ---- (b) history staging and covariance inside the rebalance ------------------------------------
def _check_weights(w, ref, hi, tag):
    err = np.abs(w - ref["w"]).max()
    print(f"{tag}: |w - ref| {err:.2e} |sum w - 1| {abs(w.sum() - 1):.2e} "
          f"ref iterations {ref['it']}")
    assert err < 1e-9, tag
    assert abs(w.sum() - 1) < 1e-12, tag
    assert np.array_equal(w <= 1e-14, ref["w"] <= 1e-14), tag
    assert np.array_equal(w >= hi - 1e-14, ref["w"] >= hi - 1e-14), tag


@pytest.mark.parametrize("name", sorted(R.COV_CASES))
def test_rebalance_history(name):
    """Books exact; weights against box_qp_weights(pairwise_cov(window)) at the project's bar;
    identical bound sets; status 0.  "tiles": the transpose skips by the dates and the window
    alone, so the first call, on the NEGATED history plane and the same context, rebalances from
    date 60 on (window start below 0: EVERY 64-date tile of the member-major scratch is staged,
    whatever an earlier test left there); the real call then needs tile 1 from date 65, and a tile
    it skipped in error keeps finite values of the wrong sign."""
    c = R.cov_case(name)
    pn = R.cov_panel()
    d = _upload(pn)
    kw = dict(A=pn["A"], top_n=c["top_n"], window=c["window"], h_range=c["h_range"], hi=R.COV_HI)
    if name == "tiles":
        assert R.TILES_FIRST[0] - c["window"] < 0 and R.TILES_FIRST[-1] == pn["T"] - 1
        first = _rebalance(dict(d, hist=-d["hist"]), R.TILES_FIRST, **kw)
        assert (first["status"] == 0).all()
    got = _rebalance(d, c["dates"], **kw)
    assert (got["status"] == 0).all(), got["status"]
    for i, rec in enumerate(c["recs"]):
        k = rec["k"]
        assert got["k"][i] == k
        _check_books(got, i, k, rec["sides"][0]["book"], rec["sides"][1]["book"])
        for side, ref in enumerate(rec["sides"]):
            _check_weights(got["weights"][i, side, :k], ref, R.COV_HI, (name, rec["t"], side))


@pytest.mark.parametrize("name", sorted(R.DEGENERATE))
def test_rebalance_degenerate_windows(name):
    """Rebalance dates 0 and 1 of a 120-date window: 0 and 1 history rows, an all-NaN covariance.
    Books over ten names: status bit 1 and NaN weights (qp_setup / qp_block); ten names: w = hi
    without a solve, status 0.  Books and union positions are exact either way."""
    top_n = R.DEGENERATE[name]
    pn = R.cov_panel()
    A = pn["A"]
    got = _rebalance(_upload(pn), (0, 1), A=A, top_n=top_n, window=120, hi=R.COV_HI)
    assert same(got["k"], np.full(2, top_n, dtype=np.int32))
    assert same(got["usize"], np.full((2, 2), A, dtype=np.int64))
    for i, t in enumerate((0, 1)):
        k, L, S = R.select(pn["pred"][t, :A], pn["trad"][t, :A], top_n)
        up = [np.stack([np.where(i == 1, bk, -1), np.where(i == 0, bk, -1)]) for bk in (L, S)]
        _check_books(got, i, k, L, S, up)
        w = got["weights"][i, :, :k]
        if top_n * R.COV_HI <= 1.0:
            assert same(w, np.full((2, k), R.COV_HI)) and got["status"][i] == 0
            assert np.isfinite(got["sums"][i]).all()
        else:
            assert np.isnan(w).all() and got["status"][i] == 1


# ---- (c) one book: afm_min_variance_weights_f64 -------------------------------------------------
def _one_book(c):
    """-> (w [k], cov [k][k], status); columns [k, ld) hold NaN, inf and 1e308"""
    import torch
    from afm import _lib
    rows, k, ld = c["rows"], c["k"], c["ld"]
    buf = np.empty((max(rows, 1), ld))
    buf[:, k:] = np.array([np.nan, np.inf, 1e308])[:ld - k]
    buf[:rows, :k] = c["R"]
    if rows == 0:
        buf[:, :k] = 0.5                                # a row the kernel must not read
    w, cov, st = _sent(R.MAX_BOOK + 1), _sent(k * k + 8), _ints((2,), torch.int32)
    _lib.run("afm_min_variance_weights_f64", _cuda(buf), rows, ld, k, float(c["lo"]),
             float(c["hi"]), w, cov, st)
    o = _host(dict(w=w, cov=cov, st=st))
    assert _untouched(o["w"][k:]) and _untouched(o["cov"][k * k:]) and o["st"][1] == ISENT
    return o["w"][:k], o["cov"][:k * k].reshape(k, k), int(o["st"][0])


@pytest.mark.parametrize("name", sorted(R.BOOK_CASES))
def test_one_book(name):
    """ld = k + 3; 0, 1 and 2 rows; both sides of the reciprocal table's end (rows 256 | 257);
    the MFMA k-step tail and 64-row chunk edge at 3, 3, 4 and 8 member tiles; a member whose
    history starts after the first chunk, and a pair without two common rows."""
    c = R.book_case(name)
    k, S = c["k"], c["S"]
    w, cov, st = _one_book(c)
    if k <= 32:
        assert np.isnan(c["R"]).any() or c["rows"] < 2
        assert same(cov, S)                            # nancorr(cov=True): bit-exact Welford
    else:
        assert np.array_equal(np.isnan(cov), np.isnan(S))
        err = np.nanmax(np.abs(cov - S)) / np.nanmax(np.abs(S))
        print(f"{name}: max |cov - S| / max|S| {err:.2e}")
        assert err <= 1e-12
    if c["rows"] < 2:
        assert np.isnan(cov).all() and st == 1 and np.isnan(w).all()
    if c.get("late"):
        assert st == 1 and np.isnan(w).all()           # a NaN entry: no solve
    if "w" in c:
        assert st == 0
        _check_weights(w, c, c["hi"], name)


# ---- (d) the PnL scan on synthetic records ------------------------------------------------------
def _scan(c, nd, spare=1):
    from afm import _lib
    out = dict(value=_sent(nd + 1 + spare), turnover=_sent(nd + spare),
               long_ret=_sent(nd + spare), short_ret=_sent(nd + spare))
    _lib.run("afm_pnl_scan_f64", nd, _cuda(c["k"]), _cuda(c["books"]), _cuda(c["sums"]),
             _cuda(c["upos"]), _cuda(c["usize"]), float(c["v0"]), float(c["rate"]), out["value"],
             out["turnover"], out["long_ret"], out["short_ret"])
    return _host(out)


def _check_scan(got, ref, n, tag):
    for key in KEYS:
        m = n + (key == "value")
        bad = np.flatnonzero(~((got[key][:m] == ref[key]) |
                               (np.isnan(got[key][:m]) & np.isnan(ref[key]))))
        assert bad.size == 0, (tag, key, "first date", int(bad[0]), got[key][bad[0]],
                               ref[key][bad[0]])
        assert _untouched(got[key][m:]), (tag, key)


@pytest.mark.parametrize("variant,nd", [("cost", nd) for nd in R.SCAN_ND] + [("wide", 65), ("tiny", 65)])
def test_pnl_scan(variant, nd):
    """value, turnover, long_ret and short_ret bit for bit against the dense recursion, over the
    first nd dates of portfolio_ref.scan_spec: chunks of 64 dates and of 12,288 record words,
    64 | 65 adds, 512 terms, books of 16 | 17 names, unions of 1 .. 32,768 ids.  "wide": rate 0,
    price sums of 1e-130 and 1e130 and a negative one (mdiv takes its IEEE division); "tiny":
    rate 0, price sums of 1e-310 and 1e300, where only that division gives the share counts."""
    c = R.scan_case(nd, variant)
    _check_scan(_scan(c, nd), c["ref"], nd, (variant, nd))


def test_pnl_scan_overlapping_books():
    """Books that share names (both thresholds inside one tie of a coarse predictor), at books of
    at most 16 names and of more.  Found while building these tests: both record kernels gave
    such a name one term per book -- two terms on one union slot, and for the one-wave kernel two
    lanes of one sort rank -- where the reference holds it short only (the short book is assigned
    last) in one slot of the sum; the long-book copy is now dropped."""
    c = R.overlap_case()
    nd = len(c["k"])
    _check_scan(_scan(c, nd), c["ref"], nd, "overlap")


def test_pnl_scan_without_dates_writes_nothing():
    got = _scan(R.scan_case(1), 0)
    assert all(_untouched(got[key]) for key in KEYS)


# ---- (e) the bootstrap: pred_bits, pair_union, both record kernels with idx, the path scan ------
_BOOT = {}


def _boot_dev(lda):
    c = R.boot_case(lda)
    d = _BOOT.get(lda)
    if d is None:
        nd = len(c["k"])
        d = _BOOT[lda] = dict(pred=_cuda(c["plane"](lda)), k=_cuda(c["k"]),
                              books=_cuda(c["books"]), sums=_cuda(c["sums"]),
                              dates=_cuda(np.arange(nd, dtype=np.int32)), nd=nd)
    return c, d


def _bootstrap(lda, paths):
    from afm import _lib
    c, d = _boot_dev(lda)
    npaths, steps = paths.shape
    out = dict(value=_sent(npaths * (steps + 1) + 1), turnover=_sent(npaths * steps + 1),
               long_ret=_sent(npaths * steps + 1), short_ret=_sent(npaths * steps + 1))
    _lib.run("afm_bootstrap_pnl_f64", lda, d["dates"], d["nd"], d["pred"], d["k"], d["books"],
             d["sums"], npaths, steps, _cuda(paths), float(c["v0"]), float(c["rate"]),
             out["value"], out["turnover"], out["long_ret"], out["short_ret"])
    got = _host(out)
    for key in KEYS:
        n = npaths * (steps + (key == "value"))
        assert _untouched(got[key][n:]), key
        got[key] = got[key][:n].reshape(npaths, -1)
    return got


@pytest.mark.parametrize("lda", R.BOOT_LDA)
@pytest.mark.parametrize("npaths", R.BOOT_NPATHS)
@pytest.mark.parametrize("steps", R.BOOT_STEPS)
def test_bootstrap_paths(steps, npaths, lda):
    """Each path bit for bit against the dense recursion over its own sequence of slots: planes
    of 1, 64 and 65 presence words and unions past 8,192; 1 .. 17 steps around the 8-date path
    chunk; the same slot twice running, a slot without books, runs of 128-name slots (one record
    per buffer), a 16-name slot followed by a 17-name slot."""
    c = R.boot_case(lda)
    paths = R.boot_paths(npaths, steps)
    got = _bootstrap(lda, paths)
    ref = R.boot_ref(c, paths)
    for key in KEYS:
        assert same(got[key], ref[key]), (key, np.argwhere(got[key] != ref[key])[:4].tolist())


@pytest.mark.parametrize("lda", R.BOOT_LDA)
def test_bootstrap_identity_path_is_the_plain_scan(lda):
    """The path 0 .. nd - 1 reproduces afm_pnl_scan_f64 on the same records (upos / usize there
    from the reference's union_positions, here from pair_union_kernel), bit for bit."""
    c = R.boot_case(lda)
    nd = len(c["k"])
    got = _bootstrap(lda, np.arange(nd, dtype=np.int32)[None, :])
    plain = _scan(c, nd, spare=0)
    ref = R.scan(c["seq"], c["v0"], c["rate"])
    for key in KEYS:
        assert same(got[key][0], plain[key]), key
        assert same(plain[key], ref[key]), key
