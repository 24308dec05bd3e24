"""afm_xs_preprocess_f64 (csrc/xsprep.hip) called directly on hand-built rows_idx / nrows and
planes (tests/xsprep_ref.py, pinned on the CPU by tests/test_xsprep_ref.py).

Bit for bit against the numpy restatement (by value, NaN patterns equal): n, lo, hi, n_lo, n_hi and
the output of a call without flags.  Steps 2 and 3 against the long-double restatement, per (date,
column): |engine - longdouble| <= max(4 E64, 16 * 2^-53 * max(1, max |ref|)), E64 the distance of
the float64 restatement from the long-double one on that item; mu and sd of info by the same
rule, each with its own E64 (behind a neutralisation of the 1e6-offset column the long-double mean
of v is itself only good to 2^-64 * 1e6, more than 16 * 2^-53).
Bit for bit as well: an item depends on its own column, the date's rows and their groups alone.

The sum of a group's neutralised values against 0: within the tolerance for a group of up to 16
rows, within tolerance * n_g / 16 for a larger one.  The outputs are doubles, each within half an
ulp of its exact value, so the sum of n_g of them is n_g * 2^-53 * max |v| away from 0 in the worst
case however exactly the mean was taken out -- and that case is real: on the two-valued column
every row of a group carries one of two rounding errors, which add up linearly (the long-double
restatement rounded to double gives the same sums; the test prints both).  16 * 2^-53 * max |ref|,
the tolerance's floor, is what 16 such roundings can reach.

The largest |engine - longdouble| / E64 per column family is printed before anything is asserted.
Measured on MI355X over all cases of this file: offset 2, small 2, ties 2, two 2, holes 2, psy 1,
normal 4 (a date of 4 rows), zeros 16 (a date of 65 rows); const and allmiss have no finite output.
A ratio above 2 is an item on which float64 happened to be nearly exact (E64 a fraction of an ulp
of the output) while the engine is one ulp of the output off; the floor of the tolerance covers
it."""
import functools

import numpy as np
import pytest

import xsprep_ref as X
from helpers import same

pytestmark = pytest.mark.gpu

SENT = -7.25
NAME = "afm_xs_preprocess_f64"
MODES = {0: (0.0, 0.0), 1: (X.MAD_C, X.MAD_C), 2: (0.05, 0.9)}
ALL_COLS = list(range(len(X.FAMILIES)))


def dev(x):
    import torch
    return torch.from_numpy(np.array(x)).to(torch.device("cuda", 0))     # (a writable copy)


def run(*args):
    from afm import _lib
    return _lib.run(NAME, *args)


@functools.lru_cache(maxsize=None)
def on_device(which):
    planes, rows_idx, nrows = X.small_case() if which == "small" else X.large_case(which)
    return dict(planes=dev(planes), rows_idx=dev(rows_idx), nrows=dev(nrows), T=len(nrows),
                lda=planes.shape[2]), (planes, rows_idx, nrows)


def prep(d, cols, dates, mode, flags, groups=None, ngroups=0, p=None, zs=None, zcols=None,
         planes=None):
    """The call on the case's buffers -> (out [K][T][lda], info [nd + 1][K][7]), both filled with
    the sentinel first."""
    import torch
    T, lda, K, nd = d["T"], d["lda"], len(cols), len(dates)
    out = torch.full((K, T, lda), SENT, dtype=torch.float64, device="cuda:0")
    info = torch.full((nd + 1, K, 7), SENT, dtype=torch.float64, device="cuda:0")
    p_lo, p_hi = MODES[mode] if p is None else p
    g = None if groups is None else dev(groups)
    run(d["planes"] if planes is None else planes, T * lda, T, lda,
        dev(np.asarray(cols, np.int32)), K, zs, None if zcols is None else dev(np.asarray(zcols, np.int32)),
        dev(np.asarray(dates, np.int32)), nd, d["rows_idx"], d["nrows"], g,
        0 if groups is None or groups.ndim == 1 else lda, ngroups, mode, p_lo, p_hi, flags, out,
        T * lda, info)
    return out.cpu().numpy(), info.cpu().numpy()


def check(got, ref, cols, dates, flags, host, what, groups=None, ngroups=0, sums=False):
    """got = (out, info) of prep; ref = X.call_ref's dict."""
    out, info = got
    planes, rows_idx, nrows = host
    K, nd = len(cols), len(dates)
    T = out.shape[1]
    rest = [t for t in range(T) if t not in set(dates)]
    assert (out[:, rest] == SENT).all(), what              # dates not evaluated: untouched
    assert (info[nd:] == SENT).all(), what
    o = out[:, dates]                                      # [K][nd][lda]
    assert (np.isnan(o) == np.isnan(ref["outld"])).all(), what   # off the rows and missing: NaN
    assert same(info[:nd, :, :5], ref["info64"][:, :, :5]), what
    worst = {}
    for i in range(nd):
        for k, c in enumerate(cols):
            r, e64 = ref["outld"][k, i], ref["E64"][i, k]
            if not np.isfinite(r).any():
                continue
            err = float(np.nanmax(np.abs(o[k, i] - r)))
            fam = X.FAMILIES[c]
            if e64 > 0 and err / e64 > worst.get(fam, (0.0,))[0]:
                worst[fam] = (err / e64, int(nrows[dates[i]]))
    print(f"xsprep {what}: largest |engine - longdouble| / E64 per family (at n rows): "
          + ", ".join(f"{f} {v:.2f} ({n})" for f, (v, n) in sorted(worst.items())))
    if flags == 0:
        assert same(o, ref["out64"]), what
    for i in range(nd):
        for k in range(K):
            r = ref["outld"][k, i]
            if np.isfinite(r).any():
                err = float(np.nanmax(np.abs(o[k, i] - r)))
                assert err <= X.tolerance(ref["E64"][i, k], r), (what, dates[i], cols[k], err)
            for j in (5, 6):                               # mu, sd
                a, b = info[i, k, j], ref["infold"][i, k, j]
                assert np.isnan(a) == np.isnan(b), (what, dates[i], cols[k], j)
                if not np.isnan(b):
                    e64 = abs(ref["info64"][i, k, j] - b)
                    assert abs(a - b) <= max(4 * e64, 16 * X.EPS * max(1.0, abs(b))), \
                        (what, dates[i], cols[k], j, a, b)
            if sums and flags == X.NEUTRALIZE:
                t = dates[i]
                idx = rows_idx[t, :nrows[t]]
                g = (groups[t] if groups.ndim == 2 else groups)[idx]
                v, vr = o[k, i, idx], r[idx]
                tol = X.tolerance(ref["E64"][i, k], r)
                for lab in np.unique(g[~np.isnan(v)]):
                    sel = (g == lab) & ~np.isnan(v)
                    s = float(np.sum(v[sel].astype(X.LD)))
                    bound = tol * max(1.0, sel.sum() / 16.0)
                    if abs(s) > 0.5 * bound:
                        print(f"xsprep {what}: group sum {s:.3e} of {sel.sum()} rows (the "
                              f"reference's: {float(np.sum(vr[sel].astype(X.LD))):.3e}), bound "
                              f"{bound:.3e}, date {t} column {cols[k]}")
                    assert abs(s) <= bound, (what, t, cols[k], int(lab), s, bound)


def both_halves(d, host, dates, mode, flags, groups=None, ngroups=0, what="", sums=False, p=None):
    """K <= 8 per call: the ten families in two calls."""
    planes, rows_idx, nrows = host
    for cols in (ALL_COLS[:8], ALL_COLS[8:] + [X.OFFSET, X.HOLES]):
        p_lo, p_hi = MODES[mode] if p is None else p
        ref = X.call_ref(planes, cols, rows_idx, nrows, dates, groups, ngroups, mode, p_lo, p_hi,
                         flags)
        got = prep(d, cols, dates, mode, flags, groups, ngroups, p=p)
        check(got, ref, cols, dates, flags, host, what, groups, ngroups, sums)


SMALL_DATES = [list(range(0, 6)), list(range(6, 11))]      # a handful of dates per call


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_row_counts_families_modes_and_flags(mode, flags):
    """0, 1, 2, 3, 4, 63, 64, 65, 511, 512 and 513 rows; the ten column families (normal, 1e6
    offset, scale 1e-4, a set of 15 values, constant, two values, NaN / +-inf sprinkled in, all
    missing, -0.0 / 0.0, and one with mad == 0); every winsor mode x both flags; seven groups with
    labels -1 and >= ngroups among them and a group of one row, one label per asset."""
    d, host = on_device("small")
    assert host[2].tolist()[:11] == X.SMALL_COUNTS
    groups = X.group_labels(np.random.default_rng(7), (d["lda"],), 7)
    for dates in SMALL_DATES:
        both_halves(d, host, dates, mode, flags, groups if flags & 1 else None, 7,
                    f"mode {mode} flags {flags}", sums=True)


@pytest.mark.parametrize("G,stride,bad", [(1, 0, False), (1, 0, True), (7, "lda", True),
                                          (256, 0, True), (256, "lda", False)])
def test_groups(G, stride, bad):
    """1, 7 and 256 groups; a group of one row; labels -1 and >= ngroups; g_stride 0 and lda (the
    labels change from date to date).  Neutralise alone (the group sums return to 0) and the full
    chain behind the MAD clip."""
    d, host = on_device("small")
    shape = (d["lda"],) if stride == 0 else (d["T"], d["lda"])
    groups = X.group_labels(np.random.default_rng(100 + G), shape, G, bad)
    for dates in SMALL_DATES:
        both_halves(d, host, dates, 0, 1, groups, G, f"G {G} stride {stride} neutralise", sums=True)
        both_halves(d, host, dates, 1, 3, groups, G, f"G {G} stride {stride} chain")


def test_quantiles_zero_and_one_clip_nothing():
    d, host = on_device("small")
    dates = [4, 7, 10]
    both_halves(d, host, dates, 2, 0, what="q = (0, 1)", p=(0.0, 1.0))
    out, info = prep(d, ALL_COLS[:8], dates, 2, 0, p=(0.0, 1.0))
    assert (info[:3, :, 3:5] == 0).all()
    raw, _ = prep(d, ALL_COLS[:8], dates, 0, 0)
    assert same(out, raw)
    both_halves(d, host, dates, 2, 2, what="q = (0.25, 0.75)", p=(0.25, 0.75))


def test_mad_zero_leaves_the_column_alone():
    d, host = on_device("small")
    dates = [7, 8, 10]
    out, info = prep(d, [X.PSY, X.ZEROS, X.NORMAL], dates, 1, 0)
    raw, _ = prep(d, [X.PSY, X.ZEROS, X.NORMAL], dates, 0, 0)
    assert same(out[:2], raw[:2]) and not same(out[2], raw[2])
    assert (info[:3, :2, 1] == -np.inf).all() and (info[:3, :2, 2] == np.inf).all()
    assert (info[:3, :2, 3:5] == 0).all() and (info[:3, 2, 3:5] > 0).any()


@pytest.mark.parametrize("n_hi", [4097, 12289, 32768])
def test_instantiation_borders_and_the_largest_date(n_hi):
    """4,096 / 4,097 and 12,288 / 12,289 rows (both sides of an instantiation's capacity) and
    32,768 rows on one date: the MAD chain with seven groups, the quantile clip alone (bit for
    bit), neutralise + standardise without a clip."""
    d, host = on_device(n_hi)
    dates = list(range(d["T"]))
    groups = X.group_labels(np.random.default_rng(n_hi), (d["lda"],), 7)
    both_halves(d, host, dates, 1, 3, groups, 7, f"n {n_hi} chain")
    both_halves(d, host, dates, 0, 1, groups, 7, f"n {n_hi} neutralise", sums=True)
    both_halves(d, host, dates, 2, 0, what=f"n {n_hi} quantile")
    both_halves(d, host, dates, 1, 0, what=f"n {n_hi} mad")
    both_halves(d, host, dates, 0, 2, what=f"n {n_hi} standardise")


def test_an_item_depends_on_its_own_inputs_only():
    """Bit for bit: K = 1 against K = 8; a permuted column list with a column named twice; a date
    subset in another order, a date twice; z on the fly from raw planes against planes of
    (x - mu) * isd made beforehand."""
    d, host = on_device("small")
    planes, rows_idx, nrows = host
    groups = X.group_labels(np.random.default_rng(7), (d["lda"],), 7)
    dates = [10, 5, 8, 3, 9]
    cols = ALL_COLS[:8]
    base, binfo = prep(d, cols, dates, 1, 3, groups, 7)
    for k in (X.NORMAL, X.OFFSET, X.HOLES):
        one, oinfo = prep(d, [k], dates, 1, 3, groups, 7)
        assert same(one[0], base[k]) and same(oinfo[:5, 0], binfo[:5, k])
    perm = [5, 2, 6, 2, 0, 1]
    got, ginfo = prep(d, perm, dates, 1, 3, groups, 7)
    assert same(got, base[perm]) and same(ginfo[:5], binfo[:5][:, perm])
    sub = [9, 10, 9]
    got, ginfo = prep(d, cols, sub, 1, 3, groups, 7)
    assert same(got[:, [9, 10]], base[:, [9, 10]])
    assert same(ginfo[:3], binfo[[4, 0, 4]])
    assert (got[:, [3, 5, 8]] == SENT).all()
    zs = X.zs_table(np.random.default_rng(3), len(X.FAMILIES), d["lda"])
    zcols = [3, 0, 1, 2, 6]
    zc = [X.NORMAL, X.OFFSET, X.TIES, X.HOLES, X.NORMAL]
    with np.errstate(all="ignore"):
        pre = np.stack([(planes[c] - zs[r][None, :, 0]) * zs[r][None, :, 1]
                        for c, r in zip(zc, zcols)])
    a, ai = prep(d, zc, dates, 1, 3, groups, 7, zs=dev(zs), zcols=zcols)
    b, bi = prep(d, list(range(5)), dates, 1, 3, groups, 7, planes=dev(pre))
    assert same(a, b) and same(ai, bi)
    assert not same(a[0], a[4])                            # one plane under two zs rows
    ident, _ = prep(d, [0, 1, 2], dates, 1, 3, groups, 7, zs=dev(zs))      # zcols = NULL: row k
    again, _ = prep(d, [0, 1, 2], dates, 1, 3, groups, 7, zs=dev(zs), zcols=[0, 1, 2])
    assert same(ident, again)
    ref = X.call_ref(planes, zc, rows_idx, nrows, dates, groups, 7, 1, X.MAD_C, X.MAD_C, 3, zs,
                     zcols)
    check((a, ai), ref, zc, dates, 3, host, "z on the fly", groups, 7)


def test_argument_errors():
    import torch
    from afm import _lib
    d, _ = on_device("small")
    T, lda = d["T"], d["lda"]
    cols, dates = dev(np.arange(3, dtype=np.int32)), dev(np.arange(4, dtype=np.int32))
    groups = dev(np.zeros(lda, dtype=np.int32))
    out = torch.full((3, T, lda), SENT, dtype=torch.float64, device="cuda:0")
    info = torch.full((4, 3, 7), SENT, dtype=torch.float64, device="cuda:0")
    good = [d["planes"], T * lda, T, lda, cols, 3, None, None, dates, 4, d["rows_idx"], d["nrows"],
            groups, 0, 7, 1, X.MAD_C, X.MAD_C, 3, out, T * lda, info]

    def bad(msg, **kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        with pytest.raises(_lib.AfmError, match=msg) as e:
            run(*a)
        assert "(-1)" in str(e.value) and NAME in str(e.value)     # AFM_E_ARG
    bad("K must be at least 1", _5=0)
    bad("bad shape", _3=lda - 32)
    bad("at most 32768", _3=32768 + 64)
    bad("unknown winsor mode", _15=3)
    bad("unknown winsor mode", _15=-1)
    bad("unknown flag bit", _18=4)
    bad("finite and positive", _16=0.0)
    bad("finite and positive", _17=-1.0)
    bad("finite and positive", _16=float("inf"))
    bad("finite and positive", _17=float("nan"))
    bad("0 <= q_lo < q_hi <= 1", _15=2, _16=0.5, _17=0.5)
    bad("0 <= q_lo < q_hi <= 1", _15=2, _16=-0.1, _17=0.5)
    bad("0 <= q_lo < q_hi <= 1", _15=2, _16=0.1, _17=1.5)
    bad("0 <= q_lo < q_hi <= 1", _15=2, _16=float("nan"), _17=0.5)
    bad("without groups", _12=None)
    bad("ngroups must be in 1..256", _14=0)
    bad("ngroups must be in 1..256", _14=257)
    bad("g_stride must be 0 or lda", _13=64)
    bad("null buffer", _0=None)
    bad("null buffer", _19=None)
    bad("null buffer", _21=None)
    bad("zcols without zs", _7=cols)
    bad("nd is negative", _9=-1)
    bad("out overlaps", _19=d["planes"])
    bad("out overlaps", _19=d["planes"][2:5])
    assert (out == SENT).all() and (info == SENT).all()    # none of them launched
    a = list(good)
    a[9] = 0
    run(*a)                                                # no dates: nothing written
    assert (out == SENT).all() and (info == SENT).all()
    a = list(good)
    a[12], a[18] = None, 2                                 # no neutralisation: groups may be NULL
    run(*a)
    run(*good)                                             # the well-formed call passes
    assert not (info == SENT).any()
    # in place on a plane the call does not read
    work = d["planes"].clone()
    a = list(good)
    a[0], a[19], a[5], a[4] = work, work[5:8], 3, cols
    run(*a)
