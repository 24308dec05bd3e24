"""The rank (Spearman) IC kernels of csrc/rankic.hip called directly on hand-built rows / rows_idx /
nrows and planes, against the integer restatement of pandas' nancorr_spearman (tests/rank_ref.py,
pinned to DataFrame.corr(method='spearman') on the CPU by tests/test_rank_ref.py).  Bit for bit,
NaN equal to NaN; no tolerance and no excluded case.  Each reference is computed once per input
set for all its planes; the column lists of the cases select from it."""
import functools

import numpy as np
import pytest

import rank_ref as K
from helpers import same

pytestmark = pytest.mark.gpu

SENT = -7.25
CAP = K.kernel_constant("kRankLdsRows")                    # rows of a date sorted in LDS
CHUNK = K.kernel_constant("kRankChunk")                    # rows per sorted chunk past that
NK = len(K.FACTOR_KINDS)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def run(name, *args):
    from afm import _lib
    return _lib.run(name, *args)


def scratch(lda):
    import torch
    from afm import _lib
    words = _lib.lib().afm_rank_scratch_words(lda)
    assert words >= 0
    return torch.empty(max(words, 1), dtype=torch.int64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def case(name: str, z: bool = False):
    """(device inputs, host ic reference [T][P][3]) of one input set, made once.
    small: 0, 1, 2, 3, 63, 64, 65, 130 and lda = 192 rows, 130 planes (every factor kind 14 times),
           dates with finite returns, with +-inf in return_2 only, with return_1 not finite on the
           special rows;
    cap:   both sides of the LDS capacity and of the sort-chunk size, one plane per kind, the last
           date with the quirk return;
    max:   one date of 32,768 rows at lda = 32,768, a tied finite column and one with +-inf."""
    if name == "small":
        counts, rets, P, lda, kinds = K.COUNTS, K.RET_OF_DATE, 130, K.LDA, K.FACTOR_KINDS
    elif name == "cap":
        edges = sorted({CAP - 1, CAP, CAP + 1, CHUNK - 1, CHUNK, CHUNK + 1})
        counts, rets = tuple(edges) + (CAP + 1,), ("fin",) * len(edges) + ("r1quirk",)
        P, lda, kinds = NK, (max(counts) + 63) // 64 * 64, K.FACTOR_KINDS
    else:
        assert name == "max"
        counts, rets, P, lda, kinds = (K.MAX_ROWS,), ("fin",), 2, K.MAX_ROWS, ("ties", "finf")
    planes, rows, rows_idx, nrows = K.rank_inputs(counts, rets, P, lda, kinds=kinds)
    zs = K.zs_table(P, lda) if z else None
    ref = K.rank_ref(planes, rows, rows_idx, nrows, zs)
    ref.setflags(write=False)
    d = dict(planes=dev(planes), rows=dev(rows), rows_idx=dev(rows_idx), nrows=dev(nrows),
             zs=dev(zs) if z else None, T=len(counts), lda=lda, host_rows=rows, counts=counts)
    return d, ref


def rank_ic(d, cols, dates=None, zcols=None, extra=2):
    """afm_rank_returns_f64 on the evaluated dates, then afm_screen_rank_ic_f64 -> ic
    [nd + extra][K][3] (the extra rows keep the sentinel when the kernel writes only its own)."""
    import torch
    T, lda = d["T"], d["lda"]
    dates = np.arange(T) if dates is None else np.asarray(dates)
    nk = len(cols)
    d_t = dev(dates.astype(np.int32))
    rrank = torch.full((3, T, lda), -1, dtype=torch.int32, device="cuda:0")
    rsum = torch.full((T, 3), -5, dtype=torch.int64, device="cuda:0")
    scr = scratch(lda)
    run("afm_rank_returns_f64", T, lda, d_t, len(dates), d["rows"], d["nrows"], rrank, rsum, scr)
    ic = torch.full((len(dates) + extra, nk, 3), SENT, dtype=torch.float64, device="cuda:0")
    run("afm_screen_rank_ic_f64", d["planes"], T * lda, T, lda, dev(np.asarray(cols, np.int32)), nk,
        d["zs"], None if zcols is None else dev(np.asarray(zcols, np.int32)), d_t, len(dates),
        d["rows"], d["rows_idx"], d["nrows"], rrank, rsum, scr, ic)
    torch.cuda.synchronize()
    return ic.cpu().numpy(), rrank.cpu().numpy(), rsum.cpu().numpy()


def column_list(nk: int):
    """nk of the 130 planes: every plane in order for 130; below that in descending order from
    plane 129 with one column repeated (all nine kinds within any nine neighbours)."""
    if nk == 130:
        return list(range(130))
    c = list(range(129, -1, -1))[:nk]
    if nk > 2:
        c[nk // 2] = c[0]
    return c


def test_reference_has_every_case():
    """The small set's reference really holds what the cases below are about: NaN ICs (constant
    columns, dates of 0 / 1 rows), and masked-path columns that differ from their clean run."""
    _, ref = case("small")
    kinds = np.array([K.FACTOR_KINDS[p % NK] for p in range(130)])
    assert np.isnan(ref[:, kinds == "const"]).all() and np.isnan(ref[:2]).all()
    assert not np.isnan(ref[4:, kinds == "finf"]).any() and not np.isnan(ref[4:, kinds == "ties"]).any()
    assert (np.abs(ref[~np.isnan(ref)]) <= 1).all()


@pytest.mark.parametrize("nk", [1, 63, 64, 65, 130])
def test_row_counts_column_counts_and_every_kind(nk):
    """0 .. 192 rows per date; no ties, heavy ties, two values, a constant, signed zeros; +-inf /
    NaN in single columns beside clean ones (a masked-path column must not disturb its
    neighbours); dates whose returns are not all finite; repeated and descending columns.
    rows_idx has gaps and the last asset; the planes' other cells must not be read."""
    d, ref = case("small")
    cols = column_list(nk)
    got, _, _ = rank_ic(d, cols)
    assert same(got[:-2], ref[:, cols, :])
    assert (got[-2:] == SENT).all()


def test_return_ranks_and_flags():
    """afm_rank_returns_f64 alone: 2 * average rank of every return on the evaluated dates, the
    sum of squared doubled deviations, -1 for a return that is not finite on the date; the other
    dates are not written."""
    d, _ = case("small")
    dates = [8, 2, 3, 5, 0, 1]
    _, rrank, rsum = rank_ic(d, [0], dates)
    rows = d["host_rows"]
    for t in range(d["T"]):
        n = d["counts"][t]
        if t not in dates:
            assert (rrank[:, t] == -1).all() and (rsum[t] == -5).all()
            continue
        for q in range(3):
            r = rows[1 + q, t, :n]
            fin = bool(np.isfinite(r).all())
            if fin:
                r2 = K.ranks2(r, np.ones(n, dtype=bool))
                assert same(rrank[q, t, :n].astype(np.int64), r2)
                assert rsum[t, q] == int(((r2 - (n + 1)) ** 2).sum())
            else:
                assert rsum[t, q] == -1
            assert (rrank[q, t, n:] == -1).all()
        assert (rsum[t] == -1).tolist() == {"fin": [False] * 3, "r2inf": [False, n > 0, False],
                                            "r1quirk": [n > 0, False, False]}[K.RET_OF_DATE[t]]


def test_lds_capacity_and_chunk_edges():
    """One below, at and one above the LDS-resident capacity and the sort-chunk size (from the
    kernel's own constants): the last LDS-resident date, the first that goes through the scratch
    in two chunks (the second of one row), every kind -- the tied columns' runs straddle the chunk
    edge -- and the quirk return on a two-chunk date.  270 columns x 4 dates: more items than
    scratch slots, so the workgroups loop."""
    d, ref = case("cap")
    assert {CAP - 1, CAP, CAP + 1, CHUNK - 1, CHUNK, CHUNK + 1} <= set(d["counts"])
    assert d["lda"] > CAP and K.kernel_constant("kRankSlots") < 270 * d["T"]
    cols = list(range(NK)) * 30
    got, _, _ = rank_ic(d, cols, extra=1)
    assert same(got[:-1], ref[:, cols, :])
    assert (got[-1] == SENT).all()
    assert not np.isnan(ref[:, K.FACTOR_KINDS.index("ties")]).any()


def test_largest_date():
    """One date of 32,768 rows at lda = 32,768, K = 2: a tied finite column (two full chunks) and
    a column with +-inf (the masked path at full length)."""
    d, ref = case("max")
    got, _, _ = rank_ic(d, [0, 1], extra=1)
    assert same(got[:-1], ref) and not np.isnan(ref).any()
    assert (got[-1] == SENT).all()


def test_z_on_the_fly():
    """zs given: z = (x - mu) * (1 / sd) from the same table in numpy; the {0, 0} row gives z = 0
    -> constant -> NaN.  zcols maps the columns to their rows; zcols = NULL is row k."""
    d, ref = case("small", True)
    cols = column_list(65)
    got, _, _ = rank_ic(d, cols, zcols=cols, extra=0)
    assert same(got, ref[:, cols, :])
    ident = list(range(70))
    got_id, _, _ = rank_ic(d, ident, extra=0)
    assert same(got_id, ref[:, ident, :])
    assert np.isnan(got_id[:, 4, :]).all() and not np.isnan(got_id[4:, 0, :]).any()
    raw, raw_ref = case("small", False)
    assert not same(ref, raw_ref)                          # ranks of z differ: mu, sd vary by row


def test_date_subset_in_descending_order():
    """The evaluated dates a subset in non-ascending order; ic rows past nd keep the sentinel."""
    d, ref = case("small")
    cols = [129, 70, 66, 66, 64, 5, 3, 3, 0]
    dates = [8, 7, 5, 3, 2, 0]
    got, _, _ = rank_ic(d, cols, dates)
    assert same(got[:len(dates)], ref[dates][:, cols, :])
    assert (got[len(dates):] == SENT).all()


def test_argument_errors():
    import torch
    from afm import _lib
    d, _ = case("small")
    T, lda = d["T"], d["lda"]
    cols, dates = dev(np.arange(3, dtype=np.int32)), dev(np.arange(T, dtype=np.int32))
    ic = torch.empty((T, 3, 3), dtype=torch.float64, device="cuda:0")
    rrank = torch.zeros((3, T, lda), dtype=torch.int32, device="cuda:0")
    rsum = torch.zeros((T, 3), dtype=torch.int64, device="cuda:0")
    scr = scratch(lda)
    pgood = [T, lda, dates, T, d["rows"], d["nrows"], rrank, rsum, scr]
    good = [d["planes"], T * lda, T, lda, cols, 3, None, None, dates, T, d["rows"], d["rows_idx"],
            d["nrows"], rrank, rsum, scr, ic]

    def bad(name, args, i, v, msg):
        a = list(args)
        a[i] = v
        with pytest.raises(_lib.AfmError, match=msg) as e:
            run(name, *a)
        assert "(-1)" in str(e.value)                      # AFM_E_ARG
    bad("afm_rank_returns_f64", pgood, 1, lda - 32, "bad shape")
    bad("afm_rank_returns_f64", pgood, 1, K.MAX_ROWS + 64, "bad shape")
    bad("afm_rank_returns_f64", pgood, 6, None, "null buffer")
    bad("afm_rank_returns_f64", pgood, 3, -1, "nd is negative")
    bad("afm_rank_returns_f64", pgood, 3, 1 << 30, "below 2\\^31")
    run("afm_rank_returns_f64", *pgood[:8], None)          # no scratch needed at this lda
    name = "afm_screen_rank_ic_f64"
    bad(name, good, 5, 0, "K must be at least 1")
    bad(name, good, 3, lda - 32, "bad shape")
    bad(name, good, 0, None, "null buffer")
    bad(name, good, 13, None, "null buffer")
    bad(name, good, 16, None, "null buffer")
    bad(name, good, 7, cols, "zcols without zs")
    bad(name, good, 9, 1 << 30, "below 2\\^31")
    with pytest.raises(_lib.AfmError, match="lda"):
        run("afm_rank_scratch_words", 100)
    big = CAP + 64                                         # past the LDS capacity: scratch needed
    a = list(good)
    a[3], a[15] = big, None
    with pytest.raises(_lib.AfmError, match="scratch"):
        run(name, *a)
    run(name, *good)                                       # the well-formed call passes
    torch.cuda.synchronize()
