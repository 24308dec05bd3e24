"""tests/portfolio_ref.py pinned to oracle/portfolio.py on every case the direct kernel tests of
tests/test_portfolio_kernels_gpu.py run (CPU only), the properties those cases claim -- term
counts, chunk closings, well-posed covariances -- asserted on the reference alone, and
include/afm.h held against the library's constants."""
import os
import re

import numpy as np
import pytest

import mv_ref
import portfolio_ref as R
from helpers import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("value", "turnover", "long_ret", "short_ret")


def _oracle_scan(seq, v0, rate):
    from oracle import portfolio as P
    with np.errstate(all="ignore"):
        return P._value_recursion(seq, rate, v0)


# ---- scan ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(R.SCAN_RUNS))
@pytest.mark.parametrize("nd", R.SCAN_ND)
def test_scan_equals_the_oracle_recursion(nd, variant):
    """Bit for bit: a mismatch means the oracle's np_sum has left numpy's order."""
    c = R.scan_case(nd, variant)
    o = _oracle_scan(c["seq"], c["v0"], c["rate"])
    for key in KEYS:
        assert same(c["ref"][key], o[key]), key
        assert c["ref"][key].shape == (nd + (key == "value"),)


@pytest.mark.parametrize("variant", sorted(R.SCAN_RUNS))
def test_scan_value_path_stays_finite(variant):
    """Cost run: finite and positive over the whole path (price sums down to 1e-2 make the
    turnover cost a sizeable part of the value).  Wide run: rate = 0, so finite whatever the
    turnover; its share counts leave 2^+-400 (mdiv's IEEE division) and one price sum is < 0."""
    c = R.scan_case(R.SCAN_LEN, variant)
    v = c["ref"]["value"]
    assert np.isfinite(v).all() and (v > 0).all()
    assert np.isfinite(c["ref"]["turnover"]).all()
    if variant == "wide":
        den = c["sums"][c["k"] > 0, 2:]
        assert (den == 1e-130).any() and (den == 1e130).any() and (den < 0).sum() == 1
        for d in (1e-130, 1e130):               # q0 = (V / 2) * RN(1 / d) and r = RN(1 / d)
            assert not 2.0 ** -400 < abs(1.0 / d) < 2.0 ** 400
    elif variant == "tiny":                     # no Markstein quotient exists for these
        den = c["sums"][c["k"] > 0, 2:]
        assert (den == 1e-310).any() and (den == 1e300).any()
        with np.errstate(all="ignore"):
            assert np.isinf(np.float64(1.0) / np.float64(1e-310))
        assert 0 < v.min() / 2 / 1e300 < 2.2250738585072014e-308    # a subnormal share count
    else:
        den = c["sums"][c["k"] > 0, 2:]
        assert den.min() >= 1e-2 and den.max() <= 1e6


def test_scan_program_holds_the_claimed_cases():
    """Book-size pairs and term counts m (adds: m - 1), union sizes, chunk closings."""
    spec = R.scan_spec()
    c = R.scan_case(R.SCAN_LEN)
    k = c["k"]
    m = np.array([R.term_count(spec, i) for i in range(R.SCAN_LEN)])
    pairs = {(int(k[i - 1]), int(k[i]), int(m[i])) for i in range(1, R.SCAN_LEN)}
    assert (16, 16, 64) in pairs             # the wave kernel and the dataflow evaluation, full
    assert {(16, 17, 65), (17, 16, 65)} & pairs and (17, 16, 66) in pairs   # nint = 64 | 65
    assert (128, 128, 512) in pairs          # kMaxTerms
    kp = {(a, b) for a, b, _ in pairs}
    assert {(0, 0), (16, 0), (0, 2), (10, 0), (0, 10)} <= kp
    assert set(k.tolist()) >= {0, 1, 2, 10, 16, 17, 64, 128}
    assert m.max() == 512
    # every union size, at a date with terms wherever two ids allow books at all
    us = c["usize"][1:, 0]
    assert set(us.tolist()) >= set(R.USIZES)
    assert set(us[m[1:] > 0].tolist()) >= set(R.USIZES) - {1}
    # members absent from the other date's set, a member kept on its side, one that flips
    assert (c["upos"][:, :, 0, :][c["books"] >= 0] == -1).any()
    kept = flipped = 0
    for i in range(1, R.SCAN_LEN):
        kept += len(np.intersect1d(spec[i - 1]["L"], spec[i]["L"]))
        flipped += len(np.intersect1d(spec[i - 1]["L"], spec[i]["S"]))
    assert kept and flipped
    # members on the summation tree's edges: slot 0, slot n - 1, both sides of a buffer edge
    term_pos = set()
    for i in range(1, R.SCAN_LEN):
        n = int(c["usize"][i, 0])
        if m[i] == 0:
            continue
        p = np.r_[c["upos"][i, :, 0, :k[i]].ravel(), c["upos"][i - 1, :, 1, :k[i - 1]].ravel()]
        term_pos |= {(n, int(x)) for x in p if x >= 0}
    missing = [(n, e) for n in R.USIZES if n >= 2 for e in (0, n - 1) if (n, e) not in term_pos]
    assert not missing, missing
    assert {(32768, 8191), (32768, 8192), (16385, 16383), (16385, 16384)} <= term_pos
    # record words: at least 3 + 2 m (header, m terms, m - 1 adds, one level), at most
    # 4 + 2 m - 1 + 64 levels.  The first 64 dates fit one 12,288-word buffer (the chunk closes
    # on its 64 DATES); from date 64 on the eight 128-name dates overflow it (it closes on WORDS)
    assert (67 + 2 * m[:64]).sum() <= 12288
    assert (k[66:74] == 128).all() and (3 + 2 * m[64:128]).sum() > 12288


def test_scan_with_overlapping_books_equals_the_oracle():
    """A name in both books is short (the short book is assigned last) and one slot of the sum;
    the case holds such names at books of at most 16 names and of more, on both dates of a pair."""
    c = R.overlap_case()
    o = _oracle_scan(c["seq"], c["v0"], c["rate"])
    for key in KEYS:
        assert same(c["ref"][key], o[key]), key
    both = [len(np.intersect1d(s["L"], s["S"])) for s in c["spec"]]
    k = c["k"].tolist()
    assert sum(b > 0 for b in both) >= 6 and any(b == 0 for b in both)
    assert any(both[i] and k[i] <= 16 and k[i - 1] <= 16 for i in range(1, len(k)))
    assert any(both[i] and both[i - 1] and k[i] > 16 for i in range(1, len(k)))
    assert np.isfinite(c["ref"]["value"]).all() and (c["ref"]["turnover"][1:] > 0).all()


# ---- select / union positions ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.selection_cases()))
def test_select_equals_the_oracle(name):
    from oracle import portfolio as P
    from oracle.xs import np_sum
    c = R.selection_cases()[name]
    A = c["A"]
    ids = np.arange(A)
    for t in range(R.SEL_T):
        p, tr = c["pred"][t, :A], c["trad"][t, :A]
        k, L, S = R.select(p, tr, c["top_n"])
        m = ~np.isnan(p)                       # the oracle sees the predicted ids only
        Lo, So = P.select_books(ids[m], p[m], tr[m], c["top_n"])
        assert k == len(Lo) and same(L, Lo) and same(S, So)
    e = R.expected_selection(c)
    assert same(np.array(e["sums"]), np.array(R.expected_selection(c, np_sum)["sums"]))
    assert np.isfinite(np.array(e["sums"])).all()


def test_selection_cases_hold_the_claimed_edges():
    cs = R.selection_cases()
    k = {n: R.expected_selection(c)["k"].tolist() for n, c in cs.items()}
    assert k["counts_0_1_2_3"] == [0, 0, 1, 1] and k["counts_19_20_21_40"] == [9, 10, 10, 10]
    assert k["top0"] == [0, 0, 0, 0]
    assert R.TIE_CAP == 4160 and R.REG_KEYS == 12288
    c = cs["tie_cap"]
    cand = (~np.isnan(c["pred"][:, :c["A"]]) & c["trad"][:, :c["A"]])
    ties = [int((cand[t] & (c["pred"][t, :c["A"]] == v)).sum())
            for t, v in enumerate((0.5, 0.5, -1.5, -1.5))]
    assert ties == [4160, 4161, 4160, 4161]
    for A in (12288, 12289):                   # the last date: both thresholds cut a tie
        c = cs[f"width{A}"]
        p, tr = c["pred"][R.SEL_T - 1, :A], c["trad"][R.SEL_T - 1, :A]
        k, L, S = R.select(p, tr, 10)
        cand = np.flatnonzero(~np.isnan(p) & tr)
        assert k == 10
        assert (p[np.setdiff1d(cand, L)] == p[L[-1]]).any()
        assert (p[np.setdiff1d(cand, S)] == p[S[-1]]).any()
    c = cs["values"]                           # +0.0 and -0.0 both in the long book's tie
    L = R.select(c["pred"][0, :c["A"]], c["trad"][0, :c["A"]], 10)[1]
    z = c["pred"][0, L[5:]]
    assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
    assert (np.diff(L[5:]) > 0).all()


def test_union_positions_layout():
    P0, P1 = np.array([2, 5, 9]), np.array([1, 5, 7, 9, 11])
    pos, n = R.union_positions(P0, P1, np.array([11, 5, 1, 9]))
    assert n == 6 and pos.tolist() == [-1, 2, -1, 4]
    pos, n = R.union_positions(None, P1, np.array([7]))
    assert n == 5 and pos.tolist() == [-1]


# ---- bootstrap ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lda", R.BOOT_LDA)
def test_bootstrap_paths_equal_the_oracle_recursion(lda):
    c = R.boot_case(lda)
    assert c["plane"](lda).shape == (len(c["k"]), lda)
    for i, s in enumerate(c["spec"]):
        assert same(np.flatnonzero(~np.isnan(c["plane"](lda)[i])), s["P"])
    paths = R.boot_paths(5, 17)
    ref = R.boot_ref(c, paths)
    for r, row in enumerate(paths):
        o = _oracle_scan([c["seq"][j] for j in row], c["v0"], c["rate"])
        for key in KEYS:
            assert same(ref[key][r], o[key]), (r, key)
    assert np.isfinite(ref["value"]).all() and (ref["value"] > 0).all()
    if lda >= 4096:
        assert set(c["k"].tolist()) >= {0, 16, 17, 128}
    if lda == 8256:
        assert c["usize"][1:, 0].max() > 8192
    p = R.boot_paths(1, 17)[0]
    kk = c["k"][p]
    assert (p[1:] == p[:-1]).any() and (kk == 0).any()
    assert any(kk[i] == min(16, c["k"].max()) and kk[i + 1] == min(17, c["k"].max())
               for i in range(16))


# ---- covariance / QP cases: asserted on the reference alone ------------------------------------
def _well_posed(S, w, it, k, lo, hi, R_):
    assert np.isfinite(S).all()
    assert np.linalg.eigvalsh(S).min() > 0
    assert k * hi > 1.0 and 1 <= it < 4 * k + 8          # a real solve that ends inside its budget
    assert ((w > lo + 1e-14) & (w < hi - 1e-14)).any()   # with a free member
    assert not mv_ref.ambiguous_bounds(w, lo, hi)
    fin = np.isfinite(R_).astype(np.int64)
    assert (fin.T @ fin).min() >= 2


@pytest.mark.parametrize("name", sorted(R.COV_CASES))
def test_rebalance_covariance_cases_are_well_posed(name):
    c = R.cov_case(name)
    for rec in c["recs"]:
        assert rec["k"] == c["top_n"]
        for s in rec["sides"]:
            assert np.isnan(s["R"]).any()              # holes: the oracle's Welford path
            _well_posed(s["S"], s["w"], s["it"], rec["k"], 0.0, R.COV_HI, s["R"])
    if name.startswith("trunc"):
        assert [len(r["sides"][0]["R"]) for r in c["recs"]] == [60, 119, 120, 120, 120]
    if name.startswith("table"):
        for s in c["recs"][0]["sides"]:                # pairs that count every row of the window
            fin = np.isfinite(s["R"]).astype(np.int64)
            assert len(s["R"]) == c["window"] and ((fin.T @ fin) == c["window"]).sum() >= 3


@pytest.mark.parametrize("name", sorted(R.BOOK_CASES))
def test_one_book_cases_are_well_posed(name):
    c = R.book_case(name)
    k, rows = c["k"], c["rows"]
    assert c["R"].shape == (rows, k)
    if rows >= 3:                                      # return-like data: |mean| <= sd per column
        with np.errstate(all="ignore"):
            assert (np.abs(np.nanmean(c["R"], axis=0)) <= np.nanstd(c["R"], axis=0, ddof=1)).all()
    if "w" in c:
        _well_posed(c["S"], c["w"], c["it"], k, c["lo"], c["hi"], c["R"])
        assert np.isnan(c["R"]).any()
        if name.startswith("table"):                   # pairs that count every row: nobs = rows
            fin = np.isfinite(c["R"]).astype(np.int64)
            assert ((fin.T @ fin) == rows).sum() >= (k - 3) ** 2
    elif rows < 2:
        assert np.isnan(c["S"]).all()
    elif rows == 2:
        bad = np.isnan(c["S"])
        assert bad[4].all() and bad[:, 4].all() and bad.sum() == 2 * k - 1
    elif c.get("late"):
        bad = np.isnan(c["S"])
        assert bad[5, 7] and bad[7, 5] and bad.sum() == 2
        assert np.isnan(c["R"][:65, 5]).all()
    else:
        assert np.isfinite(c["S"]).all() and np.isnan(c["R"]).any()
        fin = np.isfinite(c["R"]).astype(np.int64)
        assert (fin.T @ fin).min() >= 2


# ---- the header ----------------------------------------------------------------------------------
def _text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_book_cap_matches_the_library():
    from afm import portfolio
    h = _text("include", "afm.h")
    cap = int(re.search(r"#define\s+AFM_MAX_BOOK\s+(\d+)", h).group(1))
    src = _text("alpha-multi-factor-models_amd", "csrc", "portfolio.hip")
    assert cap == portfolio.MAX_BOOK == R.MAX_BOOK
    assert cap == int(re.search(r"constexpr int kMaxK = (\d+);", src).group(1))
    assert re.search(r"static_assert\(kMaxK == AFM_MAX_BOOK", src)


def test_header_status_values_match_the_kernels():
    """Only the numbers: the values afm.h lists for status[nd] are the integer literals the
    kernels and their launcher store into a status word (the behaviour behind 0 and 1 is asserted
    on the GPU, tests/test_portfolio_kernels_gpu.py)."""
    h = " ".join(_text("include", "afm.h").replace("\n *", " ").split())
    doc = re.search(r"status\[nd\] \(([^)]*)\)", h).group(1)
    documented = {int(x) for x in re.findall(r"(?:^|, )\|?(\d+) ", doc)}
    src = _text("alpha-multi-factor-models_amd", "csrc", "portfolio.hip")
    stored = set()
    for pat in (r"status\[\w+\] = (\d+);",                       # a plain store
                r"status\[\w+\] = \w+ \? (\d+) : (\d+);",        # the one-book kernel's
                r"atomicOr\(&\w+\.status\[\w+\], (\d+)\)",       # a bit of the word
                r"hipMemsetAsync\(status, (\d+),"):               # the launcher's clear
        for m in re.findall(pat, src):
            stored |= {int(x) for x in ((m,) if isinstance(m, str) else m)}
    assert documented == stored == {0, 1, 2}, (documented, stored)
