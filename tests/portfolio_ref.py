"""Plain numpy reference of the rebalance, turnover and PnL-scan kernels of csrc/portfolio.hip
(test infrastructure only: no torch, no GPU), and the cases the direct kernel tests run.

``select`` restates oracle.portfolio.select_books on asset indices; ``union_positions`` is the
layout of upos[i][side][0/1] / usize[i][0/1] described above pair_union_kernel; ``scan`` is the
KKT:864-892 value / turnover recursion evaluated DENSELY (the two union-aligned vectors, |a - b|
with NaN -> 0, np.add.reduce itself -- numpy is what the original program runs -- and IEEE
divisions), where the kernels evaluate it sparsely through a compiled summation DAG and Markstein
quotients; ``make_sequence`` turns per-date prediction sets, books and sums into the scan's
sequence, the kernels' inputs and the bootstrap's prediction plane.

tests/test_portfolio_ref.py pins all of it to oracle/portfolio.py; tests/
test_portfolio_kernels_gpu.py runs the kernels against it.  Every case list below is shared by
the two files, computed once per session and read only.
"""
from __future__ import annotations

import functools

import numpy as np

MAX_BOOK = 128                   # afm.portfolio.MAX_BOOK, AFM_MAX_BOOK, kMaxK
NP_BUF = 8192                    # numpy's reduction buffer (NPY_BUFSIZE), kNpBuf
# the tie buffer of select_top_reg in rebalance_kernel<32>: sizeof(Shared<32>::u) / sizeof(int),
# the union's largest member being hv[32][65] doubles = 32 * 65 * 8 = 16,640 bytes = 4,160 ints
# (L[528] doubles is smaller, the workgroup QP is absent from the 32-name layout).  If the struct
# changes, this edge moves: derive it again and move TIE_CAP with it.
TIE_CAP = 32 * 65 * 8 // 4
assert TIE_CAP == 4160
REG_KEYS = 48 * 256              # KR * kT: the widest panel with register-resident keys


# ---- the operations ---------------------------------------------------------------------------
def select(pred_row, trad_row, top_n: int):
    """(k, long, short): candidates = non-NaN and tradable; k = n // 2 on thin dates, else top_n;
    long descending / short ascending by prediction, ties by ascending index."""
    pred_row = np.asarray(pred_row, dtype=np.float64)
    idx = np.flatnonzero(~np.isnan(pred_row) & np.asarray(trad_row, dtype=bool))
    v = pred_row[idx]
    n = len(idx)
    k = n // 2 if n < 2 * top_n else top_n
    long_ = idx[np.lexsort((idx, -v))[:k]]
    short = idx[np.lexsort((idx, v))[:k]]
    return k, long_, short


def union_positions(P_other, P_own, members):
    """Positions of ``members`` (ids of ``P_own``) in np.union1d(P_other, P_own), -1 for a member
    absent from ``P_other`` (None: no neighbouring date, the empty set), and the union's size."""
    P_other = np.zeros(0, dtype=np.int64) if P_other is None else np.asarray(P_other)
    u = np.union1d(P_other, P_own)
    members = np.asarray(members, dtype=np.int64)
    pos = np.searchsorted(u, members)
    return np.where(np.isin(members, P_other), pos, -1).astype(np.int32), len(u)


def scan(seq, v0: float, rate: float):
    """KKT:864-892 over per-date records dict(ids (sorted), L, S, lsum, ssum, den_l, den_s)."""
    V = [np.float64(v0)]
    to_, lr, sr = [], [], []
    cur = None
    with np.errstate(all="ignore"):
        for b in seq:
            ids = np.asarray(b["ids"])
            size = V[-1] / np.float64(2)
            daily = (np.float64(b["lsum"]) - np.float64(b["ssum"])) / np.float64(2)
            new = np.full(len(ids), np.nan)
            if len(b["L"]):
                new[np.searchsorted(ids, b["L"])] = size / np.float64(b["den_l"])
            if len(b["S"]):
                new[np.searchsorted(ids, b["S"])] = -size / np.float64(b["den_s"])
            if cur is None or np.isnan(cur[1]).all():     # current_positions.dropna().empty
                to = np.float64(0)
            else:
                u = np.union1d(cur[0], ids)
                a = np.full(len(u), np.nan)
                c = np.full(len(u), np.nan)
                a[np.searchsorted(u, cur[0])] = np.nan_to_num(cur[1])
                c[np.searchsorted(u, ids)] = np.nan_to_num(new)
                d = np.abs(a - c)
                to = np.add.reduce(np.where(np.isnan(d), 0.0, d)) / np.float64(2)
            daily = daily - to * np.float64(rate) / V[-1]
            V.append(V[-1] * (np.float64(1) + daily))
            to_.append(to)
            lr.append(np.float64(b["lsum"]))
            sr.append(np.float64(b["ssum"]))
            cur = (ids, new)
    return {"value": np.array(V, dtype=np.float64), "turnover": np.array(to_, dtype=np.float64),
            "long_ret": np.array(lr, dtype=np.float64), "short_ret": np.array(sr, dtype=np.float64)}


def term_count(spec, i: int) -> int:
    """Non-zero-able slots of date i's turnover sum: members of the previous or of this date's
    books that both dates predict (the terms m of the kernels' record); 0 when no turnover."""
    if i == 0 or len(spec[i - 1]["L"]) + len(spec[i - 1]["S"]) == 0:
        return 0
    both = np.intersect1d(spec[i - 1]["P"], spec[i]["P"])
    mem = np.unique(np.concatenate([spec[i - 1]["L"], spec[i - 1]["S"], spec[i]["L"],
                                    spec[i]["S"]]).astype(np.int64))
    return int(np.isin(mem, both).sum())


def make_sequence(spec):
    """spec: per date dict(P sorted ids, L, S ids of the two books (equal length, in P),
    sums (lsum, ssum, den_l, den_s)) -> dict(seq for ``scan``; k [nd] i32, books [nd][2][128] i32
    (-1 past k), sums [nd][4], upos [nd][2][2][128] i32 (-1 past k), usize [nd][2] i64: the inputs
    of afm_pnl_scan_f64 as afm_rebalance_f64 writes them; plane(lda) -> the [nd][lda] prediction
    plane whose NaN pattern is the sets, date i in row i)."""
    nd = len(spec)
    k = np.zeros(nd, dtype=np.int32)
    books = np.full((nd, 2, MAX_BOOK), -1, dtype=np.int32)
    sums = np.zeros((nd, 4), dtype=np.float64)
    upos = np.full((nd, 2, 2, MAX_BOOK), -1, dtype=np.int32)
    usize = np.zeros((nd, 2), dtype=np.int64)
    seq = []
    for i, s in enumerate(spec):
        P = np.asarray(s["P"], dtype=np.int64)
        L, S = np.asarray(s["L"], dtype=np.int64), np.asarray(s["S"], dtype=np.int64)
        assert len(L) == len(S) <= MAX_BOOK and np.isin(L, P).all() and np.isin(S, P).all()
        k[i] = len(L)
        sums[i] = s["sums"]
        for q, j in enumerate((i - 1, i + 1)):
            other = spec[j]["P"] if 0 <= j < nd else None
            for side, bk in enumerate((L, S)):
                books[i, side, :len(bk)] = bk
                upos[i, side, q, :len(bk)], usize[i, q] = union_positions(other, P, bk)
        seq.append(dict(ids=P, L=L, S=S, lsum=sums[i, 0], ssum=sums[i, 1], den_l=sums[i, 2],
                        den_s=sums[i, 3]))

    def plane(lda: int):
        p = np.full((nd, lda), np.nan)
        for i, s in enumerate(spec):
            p[i, np.asarray(s["P"], dtype=np.int64)] = 0.25 + i
        return p
    return dict(seq=seq, k=k, books=books, sums=sums, upos=upos, usize=usize, plane=plane)


def tree_edges(n: int):
    """Slots 0 and n - 1 and both sides of every boundary of np.add.reduce's summation tree over n
    slots: the 8,192-slot buffers, the halvings (n / 2 rounded down to a multiple of 8) down to
    blocks of at most 128, and a block's body | tail edge."""
    out = set()

    def rec(lo, ln):
        out.update((lo, lo + ln - 1))
        if ln <= 128:
            body = ln - ln % 8
            out.update(p for p in (lo + body - 1, lo + body) if lo <= p < lo + ln)
            return
        n2 = ln // 2
        n2 -= n2 % 8
        rec(lo, n2)
        rec(lo + n2, ln - n2)
    for c0 in range(0, n, NP_BUF):
        rec(c0, min(NP_BUF, n - c0))
    return np.array(sorted(out), dtype=np.int64)


# ---- (d) the PnL scan's sequences --------------------------------------------------------------
USIZES = (1, 2, 7, 8, 9, 15, 16, 127, 128, 129, 135, 136, 137, 255, 256, 257, 8191, 8192, 8193,
          8199, 8200, 16384, 16385, 32768)
SCAN_ND = (1, 2, 63, 64, 65, 130)
SCAN_LEN = 130
# the first 66 dates: every union size twice running (the first pair of a size has both sets
# whole, the next one grows), small books -- their records fit one 12,288-word buffer, so the
# first chunk closes on 64 DATES; sizes of 13 dates cycle against the 48 of the union sizes
_K_A = (10, 16, 16, 17, 16, 0, 0, 2, 1, 17, 17, 10, 0)
# from date 66 on: eight 128-name dates running (a chunk that closes on WORDS), then mixed
_U_B = (8191, 8192, 8193, 8199, 8200, 16384, 16385, 32768, 256, 257)
_K_B = (128,) * 8 + (64, 64, 128, 17, 128, 16, 16, 0, 128, 64, 10, 2, 128, 128, 17, 16, 64, 0)
# dates whose books drop ONE member from the previous date's prediction set (m = 65 from 66)
_ONE_ABSENT_PAIRS = ((16, 17), (17, 16))
SCAN_SEED = 3


def _scan_shape():
    ks, ns = [], []
    for i in range(SCAN_LEN):
        if i < 66:
            n = USIZES[(i // 2) % len(USIZES)]
            # (dates 18, 19 are the only union of 129: the cycle's (0, 0) would leave it termless)
            k = {18: 2, 19: 1}.get(i, _K_A[i % len(_K_A)])
        else:
            n = _U_B[((i - 66) // 2) % len(_U_B)]
            k = _K_B[(i - 66) % len(_K_B)]
        ns.append(n)
        ks.append(min(k, n // 2))
    return ks, ns


@functools.lru_cache(maxsize=None)
def scan_spec(variant: str = "cost"):
    """The 130-date program of the scan tests (its prefixes are the shorter sequences).  ids are
    3 j + 5 for slot j of a base order; date i predicts the slots below n_i but for a few dropped
    ones (never a member of its own or a neighbouring date's books, and never a slot its
    neighbours drop, so that |P_prev U P_i| = max(n_prev, n_i) exactly).  Members sit on the
    tree's edges first (tree_edges), then anywhere; one member of the previous long book stays
    long and one flips to short where the books allow, every other member is new.
    variant "cost": price sums log-uniform in [1e-2, 1e6] (v0 = 1e8, rate = 1e-4);
    "wide": rate = 0, v0 = 1 -- price sums of 1e-130 and 1e130 (quotients outside 2^+-400: the
    IEEE division of mdiv is taken, though the Markstein quotient would still be right there)
    and one negative sum among them; "tiny": rate = 0, v0 = 1e-10 -- price sums of 1e-310 (a
    subnormal: RN(1 / d) is inf, and the Markstein quotient NaN) and 1e300 (a subnormal
    quotient): only the IEEE division of mdiv gives these share counts."""
    rng = np.random.default_rng([SCAN_SEED, 11])
    ks, ns = _scan_shape()
    books = []
    seen_absent = set()
    absent = {}                                   # date -> slot to drop from the previous set
    for i in range(SCAN_LEN):
        k, n = ks[i], ns[i]
        prev = np.concatenate(books[-1]) if books else np.zeros(0, dtype=np.int64)
        carry = []
        if i and k >= 3 and ks[i - 1] >= 3 and (ks[i - 1], k) not in ((16, 16), (128, 128)) \
                and (ks[i - 1], k) not in _ONE_ABSENT_PAIRS:
            carry = [c for c in (books[-1][0][0], books[-1][0][1]) if c < n]
        edges = rng.permutation(tree_edges(n)) if n else np.zeros(0, dtype=np.int64)
        rest = rng.permutation(n)
        ends = [p for c0 in range(0, n, NP_BUF) for p in (c0, min(c0 + NP_BUF, n) - 1)]
        cand = np.concatenate([ends[:1], ends[-1:], ends[1:-1], edges, rest]).astype(np.int64)
        _, first = np.unique(cand, return_index=True)
        cand = cand[np.sort(first)]
        fresh = cand[~np.isin(cand, prev)]
        pick = fresh if len(fresh) >= 2 * k - len(carry) else cand[~np.isin(cand, carry)]
        pick = pick[:2 * k - len(carry)]
        L = np.concatenate([carry[:1], pick[:k - len(carry[:1])]]).astype(np.int64)
        S = np.concatenate([carry[1:], pick[k - len(carry[:1]):]]).astype(np.int64)
        assert len(L) == k and len(S) == k and len(np.unique(np.r_[L, S])) == 2 * k
        books.append((L, S))
        pair = (ks[i - 1], k) if i else None
        if pair in _ONE_ABSENT_PAIRS and ns[i - 1] == n and pair not in seen_absent:
            seen_absent.add(pair)                 # the first such pair; the later ones keep all
            absent[i] = int(L[3])
    spec = []
    for i in range(SCAN_LEN):
        n = ns[i]
        lim = min(ns[max(i - 1, 0)], n, ns[min(i + 1, SCAN_LEN - 1)])
        keep = np.ones(n, dtype=bool)
        drop = np.flatnonzero((np.arange(lim) % 3 == i % 3) & (rng.random(lim) < 0.2))
        near = np.concatenate([np.concatenate(books[j]) for j in (i - 1, i, i + 1)
                               if 0 <= j < SCAN_LEN])
        keep[drop[~np.isin(drop, near)]] = False
        if i + 1 in absent:
            keep[absent[i + 1]] = False
        P = 3 * np.flatnonzero(keep).astype(np.int64) + 5
        den = 10.0 ** rng.uniform(-2, 6, 2)
        if variant != "cost":
            small, big = (1e-130, 1e130) if variant == "wide" else (1e-310, 1e300)
            den[0] = (den[0], small, big, den[0], -den[0] if i == 9 else den[0])[i % 5]
            den[1] = (big, den[1], den[1], small, den[1])[i % 5]
        lsum, ssum = rng.normal(0, 0.01, 2)
        k = ks[i]
        spec.append(dict(P=P, L=3 * books[i][0] + 5, S=3 * books[i][1] + 5,
                         sums=(lsum, ssum, den[0], den[1]) if k else (0.0, 0.0, 0.0, 0.0)))
    return tuple(spec)


SCAN_RUNS = {"cost": (1e8, 1e-4), "wide": (1.0, 0.0), "tiny": (1e-10, 0.0)}   # -> (v0, rate)


@functools.lru_cache(maxsize=None)
def scan_case(nd: int, variant: str = "cost"):
    """make_sequence of the program's first nd dates, with the reference's outputs."""
    spec = list(scan_spec(variant)[:nd])
    m = make_sequence(spec)
    v0, rate = SCAN_RUNS[variant]
    m.update(spec=spec, v0=v0, rate=rate, ref=scan(m["seq"], v0, rate))
    return m


@functools.lru_cache(maxsize=None)
def overlap_case():
    """Books that OVERLAP: predictions on two or three levels over a thin date put the long and
    the short threshold inside one tie, and both books take its lowest indices (the reference's
    nlargest / nsmallest do the same).  The reference then assigns the short book last
    (KKT:881-882), so such a name is short, and one slot of the turnover sum.  Books of at most
    16 names (the one-wave record kernel) and of more (the LDS one), selected by ``select``."""
    rng = np.random.default_rng(23)
    A, top_n = 80, 20
    spec = []
    for n, levels in ((21, 2), (21, 3), (9, 1), (40, 2), (33, 2), (41, 3), (12, 2), (21, 2),
                      (36, 1), (40, 3)):
        pred = np.full(A, np.nan)
        at = np.sort(rng.permutation(A)[:n + 6])
        pred[at] = rng.integers(0, levels, n + 6).astype(np.float64)
        trad = np.ones(A, dtype=bool)
        trad[at[rng.permutation(n + 6)[:6]]] = False
        k, L, S = select(pred, trad, top_n)
        den = 10.0 ** rng.uniform(0, 3, 2)
        lsum, ssum = rng.normal(0, 0.01, 2)
        spec.append(dict(P=np.flatnonzero(~np.isnan(pred)).astype(np.int64), L=L, S=S,
                         sums=(lsum, ssum, den[0], den[1])))
    m = make_sequence(spec)
    m.update(spec=spec, v0=1e8, rate=1e-4, ref=scan(m["seq"], 1e8, 1e-4))
    return m


# ---- (e) the bootstrap's slots and paths -------------------------------------------------------
BOOT_LDA = (64, 4096, 4160, 8256)             # 1, 64, 65 presence words; unions past 8,192
BOOT_STEPS = (1, 7, 8, 9, 17)                 # the path chunk is 8 dates
BOOT_NPATHS = (1, 5)
_BOOT_K = (16, 17, 0, 128, 128, 128, 10, 2, 1, 64, 16, 128)
# slots 3, 3: the same slot twice running; 2: k = 0; 3 3 4 5 4 .. 11 11: runs of 128-name slots
# (one record per 2,048-word buffer); 0, 1: a 16-name slot followed by a 17-name slot
_BOOT_MASTER = (3, 3, 4, 5, 4, 0, 1, 2, 6, 11, 11, 3, 9, 1, 0, 2, 7)


@functools.lru_cache(maxsize=None)
def boot_case(lda: int):
    """12 book slots on a plane of lda columns: prediction sets of ~97 % of the columns (the
    unions of two of them ~99.9 %), books of _BOOT_K names (the two at most the whole set)."""
    rng = np.random.default_rng([5, lda])
    spec = []
    for i, k0 in enumerate(_BOOT_K):
        keep = rng.random(lda) < 0.97
        keep[[0, lda - 1]] = i % 2 == 0, i % 3 != 0
        P = np.flatnonzero(keep).astype(np.int64)
        k = min(k0, len(P) // 2)
        edges = P[np.isin(P, np.r_[0, lda - 1, np.arange(63, lda, 64), np.arange(64, lda, 64),
                                   np.arange(4095, lda, 4096), np.arange(4096, lda, 4096)])]
        cand = np.concatenate([rng.permutation(edges), rng.permutation(P)])
        _, first = np.unique(cand, return_index=True)
        mem = rng.permutation(cand[np.sort(first)][:2 * k])
        den = 10.0 ** rng.uniform(-2, 6, 2)
        lsum, ssum = rng.normal(0, 0.01, 2)
        spec.append(dict(P=P, L=mem[:k], S=mem[k:],
                         sums=(lsum, ssum, den[0], den[1]) if k else (0.0, 0.0, 0.0, 0.0)))
    m = make_sequence(spec)
    m.update(spec=spec, v0=1e8, rate=1e-4)
    return m


def boot_paths(npaths: int, steps: int, nd: int = len(_BOOT_K)):
    base = np.array(_BOOT_MASTER, dtype=np.int32)
    assert base.max() < nd
    return np.stack([np.roll(base, -3 * r)[:steps] for r in range(npaths)]).astype(np.int32)


def boot_ref(case, paths):
    """every path's recursion over its own sequence of slots"""
    out = [scan([case["seq"][j] for j in row], case["v0"], case["rate"]) for row in paths]
    return {key: np.stack([o[key] for o in out]) for key in out[0]}


# ---- (a) selection panels ----------------------------------------------------------------------
SEL_T = 4
SEL_HI = 0.1
WIDTHS = (1, 2, 63, 64, 65, 255, 256, 257, 12288, 12289)


def _lda(A):
    return (A + 63) // 64 * 64


def _panel(name, A, rows, top_n=10, hi=SEL_HI, lda=None, seed=0):
    """rows: SEL_T pairs (pred [A], tradable [A]).  The pad columns [A, lda) hold finite poison
    and -inf with their tradable bits set; tmr has NaN cells; close is positive."""
    lda = _lda(A) if lda is None else lda
    rng = np.random.default_rng([seed, A, lda])
    pred = np.empty((SEL_T, lda))
    trad = np.ones((SEL_T, lda), dtype=bool)
    for t, (p, tr) in enumerate(rows):
        pred[t, :A], trad[t, :A] = p, tr
    pad = np.where(np.arange(lda - A) % 2 == 0, 1e308, -np.inf)
    pred[:, A:] = pad
    close = 50 * np.exp(rng.normal(0, 0.3, (SEL_T, lda)))
    tmr = rng.normal(0, 0.02, (SEL_T, lda))
    tmr[rng.random((SEL_T, lda)) < 0.05] = np.nan
    close[:, A:], tmr[:, A:] = pad, pad[::-1]
    hist = rng.normal(0, 0.02, (SEL_T, lda))
    hist[:, A:] = pad
    return dict(name=name, A=A, lda=lda, top_n=top_n, hi=hi, pred=pred, trad=trad, close=close,
                tmr=tmr, hist=hist)


def _random_rows(rng, A, nan=0.1, untrad=0.15):
    """normal predictions; the last date's on a grid of 0.5, so that both thresholds of a wide
    panel fall inside ties on whichever selection path its width takes"""
    rows = []
    for t in range(SEL_T):
        p = rng.normal(size=A)
        if t == SEL_T - 1:
            p = np.round(p * 2) / 2
        p[rng.random(A) < nan] = np.nan
        rows.append((p, rng.random(A) >= untrad))
    return rows


def _count_row(rng, A, n):
    """exactly n candidates; the rest split between NaN-but-tradable and predicted-untradable"""
    p = rng.normal(size=A)
    tr = np.ones(A, dtype=bool)
    out = rng.permutation(A)[n:]
    p[out[::2]] = np.nan
    tr[out[1::2]] = False
    return p, tr


def _const_row(A, ntie, value, extra=0, seed=0):
    """``ntie`` tradable assets at ``value`` spread over the width, ``extra`` distinct values above
    and as many below it, everything else NaN or untradable"""
    rng = np.random.default_rng([seed, A, ntie])
    p = np.full(A, np.nan)
    tr = np.ones(A, dtype=bool)
    at = rng.permutation(A)
    p[at[:ntie]] = value
    hi_ = at[ntie:ntie + extra]
    lo_ = at[ntie + extra:ntie + 2 * extra]
    p[hi_] = value + 1 + np.arange(extra)
    p[lo_] = value - 1 - np.arange(extra)
    other = at[ntie + 2 * extra:]
    p[other[::2]] = value                              # at the tie's value, but untradable
    tr[other[::2]] = False
    return p, tr


@functools.lru_cache(maxsize=None)
def selection_cases():
    rng = np.random.default_rng(17)
    out = []
    for A in WIDTHS:
        out.append(_panel(f"width{A}", A, _random_rows(rng, A)))
    out.append(_panel("width64_lda128", 64, _random_rows(rng, 64), lda=128))
    out.append(_panel("width256_lda320", 256, _random_rows(rng, 256), lda=320))
    # candidate counts at top_n = 10: k = 0, 0, 1, 1, 9, 10, 10 (and a full date)
    out.append(_panel("counts_0_1_2_3", 64, [_count_row(rng, 64, n) for n in (0, 1, 2, 3)]))
    out.append(_panel("counts_19_20_21_40", 64, [_count_row(rng, 64, n) for n in (19, 20, 21, 40)]))
    out.append(_panel("counts_0_21_0_0", 70, [_count_row(rng, 70, n) for n in (0, 21, 0, 0)]))
    out.append(_panel("top0", 100, _random_rows(rng, 100), top_n=0))
    # values
    A = 192
    full = np.ones(A, dtype=bool)
    z = np.full(A, np.nan)
    at = rng.permutation(A)
    z[at[:5]] = rng.uniform(1, 2, 5)
    z[at[5:10]] = -rng.uniform(1, 2, 5)
    z[at[10:40]] = np.where(np.arange(30) % 2 == 0, 0.0, -0.0)      # +0.0 and -0.0: one tie
    inf = rng.normal(size=A)
    inf[at[:2]], inf[at[2:4]] = np.inf, -np.inf
    sub = np.full(A, np.nan)
    sub[at[:25]] = np.arange(-12, 13) * 5e-324                       # subnormals around +-0
    sub[at[25:30]] = (1e-310, -1e-310, 2.2250738585072014e-308, -2.2250738585072014e-308, 0.0)
    dup = np.abs(rng.normal(size=A)) + 1
    dup[at[:4]], dup[at[4:12]] = -3.0, -2.0                          # short threshold in a tie
    out.append(_panel("values", A, [(z, full), (inf, full), (sub, full), (dup, full)]))
    big = rng.normal(size=A)
    tb = np.ones(A, dtype=bool)
    tb[np.argsort(-big)[:15]] = False                                # the largest: untradable
    nanp = rng.normal(size=A)
    nanp[rng.random(A) < 0.3] = np.nan                               # NaN with the bit set
    two = np.full(A, np.nan)
    two[at[:4]], two[at[4:104]] = 2.0, 1.0                           # need < eqtot on both sides
    exact = rng.uniform(-1, 1, A)
    exact[at[:6]], exact[at[6:10]] = 3.0, 2.0                        # eqtot == need: all_eq
    exact[at[10:13]], exact[at[13:20]] = -3.0, -2.0
    out.append(_panel("values2", A, [(big, tb), (nanp, full), (two, full), (exact, full)]))
    # ties at the capacity of the LDS tie buffer (register keys: A <= 12288), both sides
    A = REG_KEYS
    out.append(_panel("tie_cap", A, [_const_row(A, TIE_CAP, 0.5), _const_row(A, TIE_CAP + 1, 0.5),
                                     _const_row(A, TIE_CAP, -1.5, extra=3),
                                     _const_row(A, TIE_CAP + 1, -1.5, extra=3)]))
    out.append(_panel("tie_cap_top40", A, [_const_row(A, A, 0.5), _const_row(A, TIE_CAP + 1, 0.5),
                                           _const_row(A, TIE_CAP, -1.5, extra=3),
                                           _const_row(A, 2 * TIE_CAP + 1, 7.0, extra=3)],
                      top_n=40, hi=1.0 / 64))
    return {c["name"]: c for c in out}


def expected_selection(c, sum_fn=np.add.reduce):
    """k, books, sums (weights = hi: k * hi <= 1), upos, usize of a selection panel on the
    rebalance dates 0 .. SEL_T - 1.  sum_fn: the sum of nan_to_num(tmr * w) (numpy's reduce;
    tests/test_portfolio_ref.py checks the oracle's np_sum gives the same)."""
    A, hi = c["A"], c["hi"]
    sel = [select(c["pred"][t, :A], c["trad"][t, :A], c["top_n"]) for t in range(SEL_T)]
    P = [np.flatnonzero(~np.isnan(c["pred"][t, :A])) for t in range(SEL_T)]
    out = dict(k=np.array([s[0] for s in sel], dtype=np.int32), books=[], sums=[], upos=[],
               usize=[])
    for t, (k, L, S) in enumerate(sel):
        assert k * hi <= 1.0
        w = np.full(k, hi)
        s4 = [0.0, 0.0, 0.0, 0.0]
        for side, bk in enumerate((L, S)):
            s4[side] = float(sum_fn(np.nan_to_num(c["tmr"][t, bk] * w))) if k else 0.0
            den = 0
            for x in (w * c["close"][t, bk]).tolist():          # builtin sum(): 0 + x0 + x1 ...
                den = den + x
            s4[2 + side] = float(den)
        up = np.empty((2, 2, k), dtype=np.int32)
        us = [0, 0]
        for q, j in enumerate((t - 1, t + 1)):
            other = P[j] if 0 <= j < SEL_T else None
            for side, bk in enumerate((L, S)):
                up[side, q], us[q] = union_positions(other, P[t], bk)
        out["books"].append((L, S))
        out["sums"].append(s4)
        out["upos"].append(up)
        out["usize"].append(us)
    return out


# ---- (b) history staging and covariance inside the rebalance -----------------------------------
COV_A, COV_T, COV_LDA = 96, 262, 128
COV_HI = 0.1


@functools.lru_cache(maxsize=None)
def cov_panel():
    """96 assets x 262 dates: mv_ref.make_book's returns (N(0, 0.02) * U(0.5, 2) per column plus a
    1 % common factor) with a second common factor, history on every date with ~0.4 % holes;
    predictions on every date for every asset, all tradable.  Pad columns: poison, bits set."""
    import mv_ref
    rng = np.random.default_rng(2024)
    A, T, lda = COV_A, COV_T, COV_LDA
    R = mv_ref.make_book(rng, A, T, False) + rng.normal(0, 0.01, (T, 1)) * rng.normal(0, 1, A)
    present = rng.random((T, A)) >= 0.004
    pad = np.where(np.arange(lda - A) % 2 == 0, 1e308, -np.inf)

    def plane(x):
        p = np.empty((T, lda))
        p[:, :A], p[:, A:] = x, pad
        return p
    hist = plane(np.where(present, R, 1e300))          # an absent cell's value must not be read
    hb = np.ones((T, lda), dtype=bool)
    hb[:, :A] = present
    return dict(A=A, T=T, lda=lda, R=np.where(present, R, np.nan), hist=hist, hbits=hb,
                pred=plane(rng.normal(size=(T, A))), trad=np.ones((T, lda), dtype=bool),
                close=plane(50 * np.exp(rng.normal(0, 0.3, (T, A)))),
                tmr=plane(rng.normal(0, 0.02, (T, A))))


# name -> (top_n, window, h_range, rebalance dates); rows per date follow from them
COV_CASES = {}
for _n in (22, 23, 32, 33):       # one-pass | first, widest scratch-gather | first member-major
    COV_CASES[f"stage{_n}_window"] = (_n, 120, None, (200, 261))
    COV_CASES[f"stage{_n}_range"] = (_n, None, (23, 130), (200, 261))
for _n in (23, 33):               # rows 60, 119, 120, 120, 120: all >= 2 k + 8
    COV_CASES[f"trunc{_n}"] = (_n, 120, None, (60, 119, 120, 121, 261))
for _w in (255, 256, 257, 258):   # the reciprocal table ends at nobs + 1 = 257
    COV_CASES[f"table{_w}"] = (12, _w, None, (261,))
COV_CASES["tiles"] = (33, 70, None, (135, 261))     # tile 0 skipped whole, tile 1 from date 65
TILES_FIRST = (60, 261)           # the negated call before it: window start < 0, no tile skipped
DEGENERATE = {"degenerate12": 12, "degenerate40": 40, "degenerate10": 10}   # dates 0, 1


def window_rows(t, window, h_range):
    return (max(0, t - window), t) if window is not None else tuple(h_range)


@functools.lru_cache(maxsize=None)
def cov_case(name):
    """Per rebalance date and side: the book, its window's returns R, S = pairwise_cov(R) and the
    oracle's weights (w, iterations)."""
    from oracle import portfolio as P
    pn = cov_panel()
    top_n, window, h_range, dates = COV_CASES[name]
    recs = []
    for t in dates:
        k, L, S_ = select(pn["pred"][t, :pn["A"]], pn["trad"][t, :pn["A"]], top_n)
        h0, h1 = window_rows(t, window, h_range)
        sides = []
        for bk in (L, S_):
            R = pn["R"][h0:h1][:, bk]
            S = P.pairwise_cov(R)
            w, it = P.box_qp_weights(S, 0.0, COV_HI)
            sides.append(dict(book=bk, R=R, S=S, w=w, it=it))
        recs.append(dict(t=t, k=k, sides=sides))
    return dict(top_n=top_n, window=window, h_range=h_range, dates=dates, recs=recs)


# ---- (c) one book through afm_min_variance_weights_f64 -----------------------------------------
def _book(seed, k, rows, hole=0.02, hole_cols=None):
    import mv_ref
    rng = np.random.default_rng([seed, k, rows])
    R = mv_ref.make_book(rng, k, max(rows, 1), False)[:rows]
    if hole:
        at = rng.random(R.shape) < hole
        if hole_cols is not None:
            at[:, hole_cols:] = False
        R[at] = np.nan
    return R


BOOK_CASES = {}
for _k in (12, 40):
    BOOK_CASES[f"ld_k{_k}"] = dict(k=_k, rows=2 * _k + 30, ld=_k + 3)
for _r in (0, 1, 2):
    BOOK_CASES[f"rows{_r}_k12"] = dict(k=12, rows=_r)
for _r in (255, 256, 257, 258):   # holes in three columns only: the other pairs count every row
    for _k in (12, 32):
        BOOK_CASES[f"table{_r}_k{_k}"] = dict(k=_k, rows=_r, hole_cols=3)
for _r in (61, 63, 64, 65, 66, 67):
    for _k in (33, 48, 49, 128):
        BOOK_CASES[f"tail{_r}_k{_k}"] = dict(k=_k, rows=_r, cov_only=True)
BOOK_CASES["late_member_k40"] = dict(k=40, rows=100, late=True)


@functools.lru_cache(maxsize=None)
def book_case(name):
    """dict(R [rows][k], S = pairwise_cov(R), lo, hi, and w, it of box_qp_weights unless the
    case compares the covariance only)."""
    from oracle import portfolio as P
    import mv_ref
    c = dict(BOOK_CASES[name])
    k, rows = c["k"], c["rows"]
    R = _book(7, k, rows, hole_cols=c.get("hole_cols"))
    if rows == 2:                        # one hole: that member's entries are NaN, the rest finite
        R = _book(7, k, rows, hole=0)
        R[1, 4] = np.nan
    if c.get("late"):
        R[:2] = _book(7, k, rows, hole=0)[:2]          # (no other hole in member 7's two rows)
        R[:70, 5] = np.nan                # first finite value after row 64: centring constant 0
        R[2:, 7] = np.nan                 # rows 0, 1 only: no row in common with member 5
        R[:2, 7] = (0.013, -0.021)
    lo, hi = mv_ref.book_bounds(k)
    c.update(R=R, lo=lo, hi=hi, ld=c.get("ld", k))
    with np.errstate(all="ignore"):
        c["S"] = P.pairwise_cov(R) if rows else np.full((k, k), np.nan)
    if not c.get("cov_only") and rows > 2 and not c.get("late"):
        c["w"], c["it"] = P.box_qp_weights(c["S"], lo, hi)
    return c
