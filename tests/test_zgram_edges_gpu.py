"""afm_zgram_f64 and afm_zpool_f64 called directly at every tile shape and geometry edge, item by
item against the longdouble reference of tests/zgram_ref.py.

Every instantiation of zgram_kernel<NT, MODE, ZS> runs on the one small poisoned panel of
zgram_ref.make_panel: 70 dates, 192 padded assets with 150 present, the dates 29..65 (crossing bit
32 and bit 64 of the presence words), an empty date, an asset without rows; every cell outside the
row set is NaN / +-inf / 1e308 with presence bits set at random there too, so a kernel that scales
by the mask instead of selecting, or walks past a_end / the date range, yields a non-finite or a
wrong entry.  Partials become one [p+2][p+2] Gram per item through afm_gram_tree_f64 (per = 1).

The only tolerances: the derived component-wise bound 2 n 2^-53 M of zgram_ref.bound on
real-valued data, and bit equality on the exact-integer panel, between grids, between the zcols
and the natural-order statistics, and between the z-scored and the raw call on host-computed z."""
import numpy as np
import pytest

import zgram_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FF8DEAD0000BEEF                  # the prefill: a NaN payload no kernel writes
T, LDA, A_END, T0, NT = R.T, R.LDA, R.A_END, R.T0, R.NT
P_NT2 = [1, 14, 15, 30]                    # K = p + 2: 16 is one tile exactly, 32 fills both
P_NT7 = [31, 62, 94, 95, 96, 106]          # K = 33; border columns: none (<= 94), 1, 2, 12
KINDS = ["real", "int"]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


_DEV = {}


def _dev(pn):
    """the panel's device buffers (uploaded once)"""
    d = _DEV.get(id(pn))
    if d is None:
        d = _DEV[id(pn)] = dict(base=_cuda(pn.planes), cols=_cuda(pn.cols), zs=_cuda(pn.zs),
                                bits=_cuda(pn.words.view(np.int64)))
    return d


def _pe(p):
    from afm import _lib
    return _lib.lib().afm_zgram_part_bytes(p) // 8


def _sent(*shape):
    import torch
    return torch.full(shape, SENT, dtype=torch.int64, device="cuda").view(torch.float64)


def _untouched(t):
    import torch
    return bool((t.view(torch.int64) == SENT).all().item())


def _stats(pn, stats):
    """-> (zs, zcols, zid) device arguments: "nat" the panel's own rows, None the raw columns, or
    a (zs, zcols, zid) triple already on the device."""
    if stats is None:
        return None, None, 0
    if stats == "nat":
        return _dev(pn)["zs"], None, pn.p
    return stats


def _grams(p, part, nitems):
    """one [p+2][p+2] Gram per partial (the tree's final write); the spare partial behind the
    items must still hold the prefill"""
    import torch
    from afm import _lib
    G = _sent(nitems, p + 2, p + 2)
    _lib.run("afm_gram_tree_f64", p, part, nitems, 1, 1, G)
    torch.cuda.synchronize()
    assert _untouched(part[nitems]), "wrote past the last partial"
    return G.cpu().numpy()


def _zgram(pn, stats="nat", *, nblk, blk0, blk_assets, t0=T0, nt=NT, a_end=A_END, grid=0,
           planes=None):
    """afm_zgram_f64 -> (Grams [nt * nblk][K][K], part, items (t0, t1, a0, a1))"""
    from afm import _lib
    d, p = _dev(pn), pn.p
    zs, zcols, zid = _stats(pn, stats)
    base, cols, ycol = planes if planes is not None else (d["base"], d["cols"], pn.ycol)
    assert t0 + nt <= T and a_end <= LDA
    part = _sent(nt * nblk + 1, _pe(p))
    _lib.run("afm_zgram_f64", base, T * LDA, LDA, cols, zcols, p, ycol, zs, zid, d["bits"], t0, nt,
             nblk, blk0, blk_assets, a_end, part, grid)
    items = [(t0 + dd, t0 + dd + 1, blk0 + b * blk_assets, blk0 + (b + 1) * blk_assets)
             for dd in range(nt) for b in range(nblk)]
    return _grams(p, part, nt * nblk), part, items


def _zpool(pn, stats="nat", *, blk0, nrb, nchunk, t0=T0, nt=NT, a_end=A_END, grid=0):
    """afm_zpool_f64 -> (Grams [nrb * nchunk][K][K], part, items)"""
    from afm import _lib
    d, p = _dev(pn), pn.p
    zs, zcols, zid = _stats(pn, stats)
    assert t0 + nt <= T and a_end <= LDA and blk0 + 64 * nrb <= LDA
    part = _sent(nrb * nchunk + 1, _pe(p))
    _lib.run("afm_zpool_f64", d["base"], T * LDA, LDA, d["cols"], zcols, p, pn.ycol, zs, zid,
             d["bits"], t0, nt, blk0, nrb, a_end, nchunk, part, grid)
    items = [(t0 + c * nt // nchunk, t0 + (c + 1) * nt // nchunk, blk0 + 64 * r, blk0 + 64 * r + 64)
             for r in range(nrb) for c in range(nchunk)]
    return _grams(p, part, nrb * nchunk), part, items


def _check(pn, got, items, what, raw=False):
    """every item's Gram against the reference over its rows: the exact row count, symmetry,
    +0.0 everywhere for an item without rows, then bit equality (int) or the derived bound."""
    assert len(got) == len(items)
    seen_empty = False
    for i, it in enumerate(items):
        G, M, n = pn.ref(*it, raw=raw)
        g, at = got[i], (what, "item", i, "dates/assets", it)
        assert g[0, 0] == n, at + (g[0, 0], n)
        assert np.array_equal(_bits(g), _bits(g.T)), at
        if n == 0:
            seen_empty = True
            assert not _bits(g).any(), at
        elif pn.kind == "int":
            bad = np.argwhere(_bits(g) != _bits(G))
            assert len(bad) == 0, at + ("row/col", tuple(bad[0]), g[tuple(bad[0])],
                                        G[tuple(bad[0])])
        else:
            ok = np.abs(g.astype(R.LD) - G) <= R.bound(n, M)        # NaN / inf fail
            bad = np.argwhere(~ok)
            assert len(bad) == 0, at + ("row/col", tuple(bad[0]), g[tuple(bad[0])],
                                        float(G[tuple(bad[0])]), "n", n)
    return seen_empty


# ---- (a) every instantiation ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", P_NT2 + P_NT7)
def test_every_instantiation_vs_reference(p, kind):
    """<NT, 0, true>, <NT, 1, true> and, for p <= 30, <2, 0, false>: per (date, 128-asset block)
    and per (row-block, date chunk), item by item."""
    pn = R.make_panel(p, kind)
    got, _, items = _zgram(pn, nblk=2, blk0=0, blk_assets=128)
    assert _check(pn, got, items, f"zgram p={p}")                  # the empty date: zero Grams
    got, _, items = _zpool(pn, blk0=0, nrb=3, nchunk=4)
    _check(pn, got, items, f"zpool p={p}")
    if p <= 30:
        got, _, items = _zgram(pn, None, nblk=2, blk0=0, blk_assets=128)
        assert _check(pn, got, items, f"raw p={p}", raw=True)


# ---- (b) mode 0 geometry -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blk0,blk_assets", [(0, 192), (64, 128), (0, 64), (64, 64)])
@pytest.mark.parametrize("p", [30, 31, 97])
def test_mode0_geometry(p, blk0, blk_assets, kind):
    """Blocks of one, two and three row-blocks from blk0 = 0 and 64 (three: an odd count under
    the NT = 2 padding; (64, 128): the last row-block cut to 22 assets by a_end), and one block
    more than needed: it lies wholly past a_end and gives a zero Gram at every date."""
    pn = R.make_panel(p, kind)
    nblk = -(-(A_END - blk0) // blk_assets) + 1
    for stats in ("nat", None) if p <= 30 else ("nat",):
        got, _, items = _zgram(pn, stats, nblk=nblk, blk0=blk0, blk_assets=blk_assets)
        assert items[nblk - 1][2] >= A_END
        assert _check(pn, got, items, f"zgram p={p} stats={stats}", raw=stats is None)
        assert not _bits(got[nblk - 1::nblk]).any()


# ---- (c) mode 1 geometry -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("blk0,nrb", [(0, 3), (64, 2)])
@pytest.mark.parametrize("nchunk", [1, 5, 37, 50])
@pytest.mark.parametrize("p", [14, 31, 97])
def test_mode1_geometry(p, nchunk, blk0, nrb, kind):
    """One chunk, chunks that do not divide the 37 dates, one date per chunk (the empty date is
    an item of its own) and more chunks than dates (empty chunks: zero Grams)."""
    pn = R.make_panel(p, kind)
    got, _, items = _zpool(pn, blk0=blk0, nrb=nrb, nchunk=nchunk)
    empty = _check(pn, got, items, f"zpool p={p} nchunk={nchunk}")
    assert empty == (nchunk >= 37)
    if nchunk == 50:
        assert sum(t1 == t0 for t0, t1, _, _ in items) == 13 * nrb


def test_zpool_without_row_blocks_writes_nothing():
    import torch
    from afm import _lib
    pn = R.make_panel(14, "real")
    d = _dev(pn)
    part = _sent(4, _pe(14))
    _lib.run("afm_zpool_f64", d["base"], T * LDA, LDA, d["cols"], None, 14, pn.ycol, d["zs"], 14,
             d["bits"], T0, NT, 64, 0, A_END, 4, part, 0)
    torch.cuda.synchronize()
    assert _untouched(part)


# ---- (d) grid invariance -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("p", [30, 31, 100])
def test_grid_invariance(p, mode):
    """One, two and three persistent workgroups (grid = 1: one workgroup walks all 74 / 27 items:
    the item advance, the accumulator reset, the ring generations running on, the per-item
    statistics of mode 1) against the one-item-per-workgroup run of grid = 0, bit for bit.
    p = 100: two ring slots."""
    pn = R.make_panel(p, "real")

    def run(grid):
        if mode == 0:
            return _zgram(pn, nblk=2, blk0=0, blk_assets=128, grid=grid)
        return _zpool(pn, blk0=0, nrb=3, nchunk=9, grid=grid)
    ref, _, items = run(0)
    assert len(items) >= 24
    _check(pn, ref, items, f"mode {mode} p={p} grid=0")
    for grid in (1, 2, 3):
        got, _, _ = run(grid)
        bad = np.argwhere(_bits(got) != _bits(ref))
        assert len(bad) == 0, (f"mode {mode} p={p} grid={grid}", "item/row/col", tuple(bad[0]))


# ---- (e) zcols -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", [15, 30, 62, 96])
def test_zcols(p, kind):
    """Statistics behind zcols (p + 5 rows, a random injection, the identity row in the middle,
    the unused rows NaN): the reference, the natural-order call, and -- p <= 30 -- the raw call on
    planes that hold the host-computed (x - mu) * rs."""
    import torch
    pn = R.make_panel(p, kind)
    zs, zcols, zid = R.scattered_stats(pn)
    stats = (_cuda(zs), _cuda(zcols), zid)
    for call, kw in ((_zgram, dict(nblk=2, blk0=0, blk_assets=128)),
                     (_zpool, dict(blk0=0, nrb=3, nchunk=5))):
        got, part, items = call(pn, stats, **kw)
        _check(pn, got, items, f"{call.__name__} zcols p={p}")
        nat, _, _ = call(pn, "nat", **kw)
        assert np.array_equal(_bits(got), _bits(nat)), call.__name__
    if p <= 30:
        planes = (_cuda(pn.zplanes()), torch.arange(p, dtype=torch.int32, device="cuda"), p)
        kw = dict(nblk=2, blk0=0, blk_assets=128)
        got, part, items = _zgram(pn, stats, **kw)
        raw, rpart, _ = _zgram(pn, None, planes=planes, **kw)
        assert np.array_equal(_bits(got), _bits(raw))
        assert torch.equal(part.view(torch.int64), rpart.view(torch.int64))   # the partials too


# ---- (f) rejections ------------------------------------------------------------------------------
_ZGRAM_OK = dict(p=14, lda=LDA, blk0=0, a_end=A_END, blk_assets=64, nblk=3, zs=True, bits=True)
_ZPOOL_OK = dict(p=14, lda=LDA, blk0=0, a_end=A_END, nrb=3, nchunk=4, zs=True, bits=True)


@pytest.mark.parametrize("entry,bad", [
    ("afm_zgram_f64", dict(p=0)), ("afm_zgram_f64", dict(p=107)),
    ("afm_zpool_f64", dict(p=0)), ("afm_zpool_f64", dict(p=107)),
    ("afm_zgram_f64", dict(lda=100)), ("afm_zpool_f64", dict(lda=100)),
    ("afm_zgram_f64", dict(blk0=32)), ("afm_zpool_f64", dict(blk0=32)),
    ("afm_zgram_f64", dict(a_end=LDA + 1)), ("afm_zpool_f64", dict(a_end=LDA + 1)),
    ("afm_zgram_f64", dict(blk_assets=96)), ("afm_zgram_f64", dict(nblk=0)),
    ("afm_zpool_f64", dict(nchunk=0)), ("afm_zpool_f64", dict(zs=None)),
    ("afm_zgram_f64", dict(bits=None)), ("afm_zpool_f64", dict(bits=None)),
], ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_rejections(entry, bad):
    """A bad argument is an AfmError naming the entry point, and part keeps its prefill."""
    import torch
    from afm import _lib
    pn = R.make_panel(106, "real")                      # buffers large enough for any p passed
    d = _dev(pn)
    a = dict(_ZGRAM_OK if entry == "afm_zgram_f64" else _ZPOOL_OK, **bad)
    zs = d["zs"] if a["zs"] else None
    bits = d["bits"] if a["bits"] else None
    part = _sent(NT * 3 + 1, _pe(106))
    head = (d["base"], T * LDA, a["lda"], d["cols"], None, a["p"], pn.ycol, zs, a["p"], bits, T0,
            NT)
    if entry == "afm_zgram_f64":
        tail = (a["nblk"], a["blk0"], a["blk_assets"], a["a_end"], part, 0)
    else:
        tail = (a["blk0"], a["nrb"], a["a_end"], a["nchunk"], part, 0)
    with pytest.raises(_lib.AfmError, match=entry):
        _lib.run(entry, *head, *tail)
    torch.cuda.synchronize()
    assert _untouched(part)


# ---- (g) no dates --------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [14, 97])
def test_no_dates(p):
    """nt = 0 (at a date inside the panel): afm_zgram_f64 owns no partial and writes nothing;
    afm_zpool_f64 owns nrb * nchunk partials, each the empty sum: all zero."""
    import torch
    from afm import _lib
    pn = R.make_panel(p, "real")
    d = _dev(pn)
    part = _sent(13, _pe(p))
    head = (d["base"], T * LDA, LDA, d["cols"], None, p, pn.ycol, d["zs"], p, d["bits"], T - 1, 0)
    _lib.run("afm_zgram_f64", *head, 3, 0, 64, A_END, part, 0)
    torch.cuda.synchronize()
    assert _untouched(part)
    _lib.run("afm_zpool_f64", *head, 0, 3, A_END, 4, part, 0)
    torch.cuda.synchronize()
    assert not part[:12].view(torch.int64).any().item()
    assert _untouched(part[12])
    assert not _bits(_grams(p, part, 12)).any()
