"""The fused launches of the step's seams (include/afm_seams.h) against the launches they replace,
bit for bit (``torch.equal`` on the int64 view) on the same random leaves and panels:

* afm_gram_tree3_f64 against three afm_gram_tree_f64 levels;
* afm_gram_final_f64 against two final trees + afm_vec_add_f64;
* afm_ols_solve_parts_f64 against the final tree + afm_ols_solve_f64;
* afm_factors_rows_f64 against afm_factors_f64 + two afm_drop_last_obs_bits;
* afm_zstats_rows_f64 against afm_zstats_finalize_f64 + afm_row_bits;
* Pipeline.step() with the FM Grams forked at the pooled kernel against the other placements.

The leaves hold +-0.0, subnormals and 1e300-scale values, so a reordered or an extra addition
(-0.0 + 0.0, a lost subnormal) shows in the bits.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C1, C2 = 32, 2                      # the pipeline's chunk tree (N_CHUNKS = 64)
NRB_MAX = 21


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64)


def _same(a, b, what=""):
    import torch
    assert torch.equal(_bits(a), _bits(b)), what


def _pe(p):
    import torch  # noqa: F401  (before the library loads: one HIP runtime in the process)
    from afm import _lib
    return _lib.lib().afm_zgram_part_bytes(p) // 8


def _rough(shape, seed, sym_tiles=0):
    """Doubles whose sums depend on the order: mixed signs over the scales 1e300, 1, 1e-300 and
    the subnormals, with exact +-0.0 among them.  ``sym_tiles``: the tile count of partials
    [...][part] whose diagonal tiles are made symmetric, as a Gram's are (tile pair (i, j) of the
    j-major upper-triangle list is 256 doubles, row-major 16 x 16; a final tree writes both
    halves of a diagonal tile to the same entries)."""
    import torch
    rng = np.random.default_rng(seed)
    v = rng.normal(size=shape) * rng.choice([1e300, 1.0, 1e-300, 5e-324 * 1000], size=shape)
    k = rng.integers(0, 16, size=shape)
    v[k == 0] = 0.0
    v[k == 1] = -0.0
    for j in range(sym_tiles):
        q = j * (j + 1) // 2 + j
        tile = v[..., q * 256:(q + 1) * 256].reshape(shape[:-1] + (16, 16))
        lo = np.tril_indices(16, -1)
        tile[..., lo[0], lo[1]] = tile[..., lo[1], lo[0]]
        v[..., q * 256:(q + 1) * 256] = tile.reshape(shape[:-1] + (256,))
    return torch.from_numpy(v).cuda()


@pytest.fixture(scope="module")
def leaves():
    """p -> the pooled leaves [NRB_MAX][C2 * C1][part] (a case reads its first nrb row-blocks)."""
    return {p: _rough((NRB_MAX, C1 * C2, _pe(p)), seed=p) for p in (97, 30)}


@pytest.mark.parametrize("rb_per_blk", [1, 20, 32])
@pytest.mark.parametrize("nrb", [1, 3, 20, 21])
@pytest.mark.parametrize("p", [97, 30])
def test_tree3_matches_three_levels(leaves, p, nrb, rb_per_blk):
    import torch
    from afm import _lib
    pe = _pe(p)
    part = leaves[p][:nrb]
    nblk = -(-nrb // rb_per_blk) + 1                     # + a block past the last row-block
    opt = dict(dtype=torch.float64, device="cuda")
    c1b, rb = torch.empty((nrb * C2, pe), **opt), torch.empty((nrb, pe), **opt)
    ref = torch.zeros((nblk, pe), **opt)
    _lib.run("afm_gram_tree_f64", p, part, nrb * C1 * C2, C1, 0, c1b)
    _lib.run("afm_gram_tree_f64", p, c1b, nrb * C2, C2, 0, rb)
    _lib.run("afm_gram_tree_f64", p, rb, nrb, rb_per_blk, 0, ref)
    got = torch.full((nblk, pe), float("nan"), **opt)
    _lib.run("afm_gram_tree3_f64", p, part, nrb, C1, C2, rb_per_blk, nblk, got)
    torch.cuda.synchronize()
    _same(got, ref)
    assert not _bits(got[-1]).any()                      # the empty block: +0.0


def test_tree3_rejects_bad_shapes(leaves):
    import torch
    from afm import _lib
    out = torch.empty((2, _pe(30)), dtype=torch.float64, device="cuda")
    for c1, c2, rbb, nblk in ((33, 2, 1, 2), (32, 3, 32, 2), (32, 2, 1, 1)):
        with pytest.raises(_lib.AfmError, match="afm_gram_tree3_f64"):
            _lib.run("afm_gram_tree3_f64", 30, leaves[30], 2, c1, c2, rbb, nblk, out)


@pytest.mark.parametrize("nte", [0, 1, 2, 8])
@pytest.mark.parametrize("p", [97, 30])
def test_final_matches_trees_and_add(p, nte):
    import torch
    from afm import _lib
    nblk, pe, p2 = 8, _pe(p), p + 2
    nt = 7 if p == 97 else 2
    blocks = _rough((nblk, pe), seed=100 + p, sym_tiles=nt)
    te = _rough((max(nte, 1), pe), seed=200 + p + nte, sym_tiles=nt)
    opt = dict(dtype=torch.float64, device="cuda")
    ref, ref_te = torch.full((1, p2, p2), float("nan"), **opt), torch.zeros((1, p2, p2), **opt)
    _lib.run("afm_gram_tree_f64", p, blocks, nblk, nblk, 1, ref)
    if nte:
        _lib.run("afm_gram_tree_f64", p, te, nte, nte, 1, ref_te)
        _lib.run("afm_vec_add_f64", p2 * p2, ref_te, ref)
    got, got_te = torch.full((1, p2, p2), float("nan"), **opt), torch.zeros((1, p2, p2), **opt)
    _lib.run("afm_gram_final_f64", p, blocks, nblk, te if nte else None, nte, got, got_te)
    torch.cuda.synchronize()
    _same(got, ref, "gram")
    _same(got_te, ref_te, "te_gram")


@pytest.fixture(scope="module")
def fm_parts():
    """W -> per-date partial Grams [5][W][part] of a 30-regressor design on W asset blocks: date 1
    rank-deficient (a regressor constant over the cross-section), date 3 without rows."""
    import torch
    from afm import _lib
    pf, T = 30, 5
    out = {}
    for W in (1, 2, 8):
        lda = 64 * W
        rng = np.random.default_rng(40 + W)
        base = rng.normal(1.0, 2.0, size=(pf + 1, T, lda))
        base[4, 1] = 3.25
        keep = rng.random((T, lda)) < 0.9
        keep[:, lda - 10:] = False
        keep[3] = False
        words = np.zeros((1, lda), np.uint64)
        for t in range(T):
            words[0] |= keep[t].astype(np.uint64) << np.uint64(t)
        cols = torch.arange(pf, dtype=torch.int32, device="cuda")
        part = torch.full((T, W, _pe(pf)), float("nan"), dtype=torch.float64, device="cuda")
        _lib.run("afm_zgram_f64", torch.from_numpy(base).cuda(), T * lda, lda, cols, None, pf, pf,
                 None, 0, torch.from_numpy(words.view(np.int64)).cuda(), 0, T, W, 0, 64, lda - 10,
                 part, 0)
        out[W] = part
    return out


@pytest.mark.parametrize("W", [1, 2, 8])
@pytest.mark.parametrize("fnd", [1, 5])
def test_solve_parts_matches_tree_and_solve(fm_parts, fnd, W):
    import torch
    from afm import _lib
    pf, tol = 30, 1e-10
    part = fm_parts[W][:fnd]
    opt = dict(dtype=torch.float64, device="cuda")
    shift = torch.zeros((fnd, pf + 2), **opt)
    gram = torch.empty((fnd, pf + 2, pf + 2), **opt)

    def outs():
        return (torch.full((fnd, pf + 1), 7.0, **opt), torch.full((fnd,), -1.0, **opt),
                torch.full((fnd,), -1, dtype=torch.int32, device="cuda"))
    ref, got = outs(), outs()
    _lib.run("afm_gram_tree_f64", pf, part, fnd * W, W, 1, gram)
    _lib.run("afm_ols_solve_f64", gram, shift, pf, fnd, tol, *ref)
    _lib.run("afm_ols_solve_parts_f64", part, W, shift, pf, fnd, tol, *got)
    torch.cuda.synchronize()
    for a, b, what in zip(got, ref, ("beta", "nobs", "rank")):
        assert torch.equal(a if a.dtype is torch.int32 else _bits(a),
                           b if b.dtype is torch.int32 else _bits(b)), what
    rank = ref[2].cpu().numpy()
    assert rank[0] == pf                                  # the cases are what they claim to be
    if fnd == 5:
        assert rank[1] == pf - 1 and rank[3] == 0 and ref[1][3].item() == 0.0
        assert torch.isnan(ref[0][3]).all()


def test_factor_rows_match_masks_and_last_obs():
    """A 130 x 200 ragged panel: an asset present on the last date, one whose last observation is
    mid-series (the short-lived asset), one never present, and the lda padding lanes."""
    import torch
    import afm
    from afm import _lib
    from afm.factors import N_FACTORS
    from afm.synthetic import make_panel
    p = make_panel(130, 200, seed=11, edge_cases=True, hole_frac=0.01)
    p.valid[:, 7] = False                                 # an asset with no observation
    assert p.valid[-1].any() and p.valid[:, 3].any() and not p.valid[-1, 3] and p.lda == 192
    g = afm.PanelGrid.from_panel(p)
    T, A, lda, nch = g.T, g.A, g.lda, (g.T + 63) // 64
    f64 = dict(dtype=torch.float64, device="cuda")

    def words():
        return torch.full((nch, lda), -1, dtype=torch.int64, device="cuda")
    out_r, out_g = (torch.full((N_FACTORS, T, lda), float("nan"), **f64) for _ in range(2))
    nf_r, fi_r, ad_r, fr_r = (words() for _ in range(4))
    nf_g, fi_g, ad_g, fr_g = (words() for _ in range(4))
    _lib.run("afm_factors_f64", T, A, lda, g.close, g.volume, g.ret1d, g.excess, g.vbits, out_r,
             nf_r, fi_r)
    _lib.run("afm_drop_last_obs_bits", T, lda, g.vbits, nf_r, ad_r)
    _lib.run("afm_drop_last_obs_bits", T, lda, g.vbits, fi_r, fr_r)
    _lib.run("afm_factors_rows_f64", T, A, lda, g.close, g.volume, g.ret1d, g.excess, g.vbits,
             out_g, nf_g, fi_g, ad_g, fr_g)
    torch.cuda.synchronize()
    for a, b, what in ((out_g, out_r, "out"), (nf_g, nf_r, "nanfree"), (fi_g, fi_r, "finite"),
                       (ad_g, ad_r, "alldf"), (fr_g, fr_r, "frows")):
        _same(a, b, what)
    assert not ad_g[:, A:].any() and not ad_g[:, 7].any()      # padding lanes, the absent asset
    assert (nf_g != ad_g).any().item()                          # last observations were dropped


@pytest.mark.parametrize("t0,t1", [(0, 192), (5, 130), (70, 100), (64, 128)])
def test_zstats_rows_match_finalize_and_row_bits(t0, t1):
    import torch
    from afm import _lib
    K, lda, nch = 7, 320, 3
    rng = np.random.default_rng(5)
    mu, sd = rng.normal(size=(K, lda)), rng.uniform(0.1, 3.0, size=(K, lda))
    sd[2, 9] = 0.0                                        # sigma = 0
    mu[5, 70] = np.nan                                    # a NaN mean
    sd[0, 300] = 1e-320                                   # 1 / sigma overflows
    mu, sd = torch.from_numpy(mu).cuda(), torch.from_numpy(sd).cuda()
    rows = torch.from_numpy(rng.integers(-2**63, 2**63 - 1, size=(nch, lda))).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")

    def outs():
        return (torch.full((K + 1, lda, 2), float("nan"), **f64),
                torch.full((lda,), -1, dtype=torch.int32, device="cuda"),
                torch.full((nch, lda), -1, dtype=torch.int64, device="cuda"))
    (zs_r, ok_r, out_r), (zs_g, ok_g, out_g) = outs(), outs()
    _lib.run("afm_zstats_finalize_f64", mu, sd, K, lda, zs_r, ok_r)
    _lib.run("afm_row_bits", nch, lda, rows, None, ok_r, t0, t1, out_r)
    _lib.run("afm_zstats_rows_f64", mu, sd, K, lda, zs_g, ok_g, nch, rows, t0, t1, out_g)
    torch.cuda.synchronize()
    _same(zs_g, zs_r, "zs")
    assert torch.equal(ok_g, ok_r) and torch.equal(out_g, out_r)
    assert ok_r.sum().item() == lda - 3 and not out_g[:, [9, 70, 300]].any()


def test_step_fm_fork_at_pool_bit_identical():
    """300 assets x 900 dates (train_end a trading date: its Gram is added twice): the step with
    the FM Grams forked at the pooled kernel, the default, fm_fork='predict', and the one-pass
    factor stage (the streamed stage is this grid's default) leave bitwise the same results."""
    import torch
    import afm
    from afm.pipeline import Pipeline, PipelineConfig
    from afm.synthetic import make_panel
    grid = afm.PanelGrid.from_panel(make_panel(300, 900, seed=3, tradable_p=0.9))
    runs = []
    for place in ({}, {"fm_fork": "pool"}, {"fm_fork": "predict"},
                  {"fm_fork": "pool", "zstats_slabs": 0}):
        pipe = Pipeline(grid, PipelineConfig(train_end="2002-05-31", valid_end="2002-10-04",
                                             **place))
        pipe.step()
        runs.append(pipe)
    torch.cuda.synchronize()
    ref = runs[0]
    assert ref.sp.dup and ref.stream_z and not runs[3].stream_z
    assert int(ref.pool_g[0, 0, 0].item()) > 10000 and (ref.fm_rank > 0).sum().item() > 500
    for other in runs[1:]:
        for name in ("pool_g", "te_gram", "lasso_beta", "pred", "fm_beta", "fm_nobs", "fm_mean",
                     "fm_t", "zrows", "alldf", "zs"):
            _same(getattr(other, name), getattr(ref, name), name)
        assert torch.equal(other.fm_rank, ref.fm_rank)
        for k, v in ref.reb.items():
            assert torch.equal(_bits(other.reb[k]) if v.dtype is torch.float64 else other.reb[k],
                               _bits(v) if v.dtype is torch.float64 else v), k
        for k, v in ref.pnl.items():
            _same(other.pnl[k], v, k)
