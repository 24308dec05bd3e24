"""The reference's hot path, end to end on one device (BASELINE.json ``metric``; SURVEY.md §8(a)
rows I0-I16, A1-A4, R1, K1-K4): the notebook chain that feeds ``PortfolioManager``.

One ``step()`` over a device-resident calendar-grid panel:

1. factors      afm_factors_f64: the 98 No-talib.py columns (NT:1-93); all_df rows = the NT:33
                dropna rows (label planes non-NaN)
2. zstats       train-window per-security mean / std of the 97 feature columns (KKT:424-451:
                train = dates <= train_end, features = Index.difference order, KKT:433-443 --
                tmr_ret1d included, as in the reference); assets with a non-finite mean or a
                zero / NaN std drop out entirely (their z is NaN in every row, KKT:452-454)
3. xs_gram      the pooled Gram of [1, z_1..z_97, target] over every train + valid row, on fp64
                MFMA with z computed on the fly (afm_zpool_f64: one partial per 64-asset row-block
                and date chunk, summed over a fixed tree -- row-blocks within the 8 asset blocks,
                then the blocks -- so it is bit-identical for any GPU count).  The inclusive
                .loc slices of KKT:426-427 put train_end in train AND valid: its Gram is added
                once more.
4. lasso        Lasso(alpha=2e-4, max_iter=10000).fit (KKT:605-607) by Gram coordinate descent
5. predict      lasso.predict on the test dates (KKT:612), z on the fly
6. rebalance    PortfolioManager(lasso_predict, ...).calculate_portfolio() (KKT:976-977):
                per test date top/bottom-n books, rolling-window pairwise covariance of the
                target history (north star: 252 dates; None = the reference's whole
                training window), exact box-QP weights (SLSQP's problem, KKT:811-833)
7. pnl          value / turnover recursion (KKT:864-892)
side streams:
8. analyzer     AlphaSignalAnalyzer(lasso_predict, price_data=df_test close).run() (KKT:630-631):
                forward returns, IC, decile layers, top-10 backtest, IR
9. fm           the north-star extension: classic Fama-MacBeth -- per-date Grams of
                [1, FM30 factor values, target] over the same rows (afm_zgram_f64: per (date,
                asset block) partials, fixed tree), per-date cross-sectional OLS, mean / t.
                FM30 is a stated well-conditioned subset of the 97 features (worst date
                cond(corr) ~3e2 on config A, raw or z-scored).

The reference's LinearRegression over all 97 columns (KKT:582-583) is not a stage: that design
is numerically rank-deficient (cond ~1e10 measured on config A: BBANDS_upper + BBANDS_lower =
2 SMA before z-scoring, and the price-level columns are nearly collinear after), so its
coefficients carry ~1e-6 relative noise even in scikit-learn's SVD solve and no implementation
can be checked against another.  The portfolio consumes the Lasso predictions (KKT:976) --
a well-posed fit -- and that chain is what a step runs.  ``afm.LinearRegression`` remains the
drop-in for well-conditioned designs.

All buffers are allocated once; a step does no host synchronisation.
"""
from __future__ import annotations

import operator
from dataclasses import dataclass

import numpy as np

from . import _lib
from .factors import COL, FACTOR_NAMES, N_FACTORS, TARGET, TMR
from .grid import PanelGrid
from .portfolio import MAX_BOOK

# KKT:433-443: every column except the raw inputs and `target`, in Index.difference (sorted)
# order -- the 96 factors and tmr_ret1d
FEATURES = sorted(n for n in FACTOR_NAMES if n != "target")
# Fama-MacBeth design (the north-star per-date regression): 30 z-scored columns chosen greedily
# for the smallest worst-date condition number on the config-A synthetic panel (worst sampled
# date cond(corr) ~ 3e2; the full 97-column design is ~1e10 pooled, singular per date)
FM30 = ["tmr_ret1d", "ACCEL_32", "sd5_15", "corr_5", "OBV", "sd_15", "MOM_38", "volsd5_15",
        "vol_change", "volsd_15", "corr_15", "ACCEL_38", "BBANDS_upper_14", "ACCEL_20",
        "ACCEL_26", "ROCR_14", "sd_3", "ACCEL_50", "volsd_3", "ACCEL_44", "ACCEL_56", "ROCR_20",
        "ROCR_56", "PVT", "PSY", "ROCR_32", "MOM_26", "ACCEL_14", "RSI_8", "MOM_50"]
# a non-reference variant of KKT:433-443 (bench.py's "dense_lasso" line): the 96 factors without
# tmr_ret1d.  With tmr_ret1d in the design the Lasso keeps one coefficient (the headline step
# reads one plane in the predict); without it the fit is dense.
DENSE_FEATURES = tuple(n for n in FEATURES if n != "tmr_ret1d")
# ... and a smaller Lasso penalty (KKT:605 uses 2e-4): on the synthetic panels the 96-column fit
# keeps 1 coefficient at 2e-4 and ~24 at 2e-6 (config-A-sized check with the oracle's CD)
DENSE_ALPHA = 2e-6
N_BLOCKS = 8           # fixed asset blocks of the Gram trees (>= the largest GPU count)
N_CHUNKS = 64          # date chunks of the pooled Gram's row-block partials (2 tree levels)
CHUNK_TREE = (32, 2)   # the chunks of a row-block: groups of 32, then the 2 results

STAGES = ("factors", "zstats", "xs_gram", "lasso", "predict", "rebalance", "pnl", "fm",
          "analyzer")
PIPELINE_STAGES = STAGES
EXCHANGE_STAGES = STAGES + ("exchange",)
# optional step() events around single launches (bench.py's rooflines): the one-pass factor call
# (factor_panel_kernel + masks_kernel) and the pooled Gram's partial kernel (zgram_kernel<7, 1>)
KERNEL_MARKS = ("k_factor", "k_gram")


@dataclass
class PipelineConfig:
    train_end: str = "2015-12-31"   # KKT:424
    valid_end: str = "2016-12-31"   # KKT:425
    alpha: float = 2e-4             # KKT:605
    max_iter: int = 10000           # KKT:605
    lasso_tol: float = 1e-4         # sklearn Lasso default
    fm_features: tuple = tuple(FM30)
    top_n: int = 10                 # KKT:796
    window: int | None = 252        # rolling covariance window (north star); None = KKT:858
    lo: float = 0.0                 # KKT:828
    hi: float = 0.1
    # the return term of the weight solve: min 1/2 w'Sw - risk_tolerance * s * mu'w (s = -1 for
    # the short book); 0 = the min-variance solve.  expected: "prediction" (mu = the step's
    # predictions) or "history" (the members' means over the covariance window, KKT:821)
    risk_tolerance: float = 0.0
    expected: str = "prediction"
    rate: float = 1e-4              # KKT:796
    v0: float = 100000000.0         # KKT:804
    tol: float = 1e-10              # pivot threshold of the per-date solve
    analyzer: bool = True
    # the regression design: None = the reference's 97 columns (KKT:433-443, FEATURES).  A stated
    # variant may name another subset -- e.g. DENSE_FEATURES, which drops tmr_ret1d (the
    # undemeaned twin of the target, NT:90-91) so the Lasso keeps many coefficients
    features: tuple | None = None
    # stream placement (moves work between streams only; the outputs are bitwise the same):
    # labels_side -- one GPU: the two label planes on a side stream beside the factor kernel;
    # fm_fork -- one GPU: where the FM per-date Grams fork off the main stream ("pool": straight
    # after the pooled Gram's partial kernel, ahead of its trees; "gram", "predict", "analyzer" or
    # "rebalance": after that stage); main_priority -- the main stream at high priority
    labels_side: bool = True
    fm_fork: str = "predict"
    main_priority: bool = True
    # fm_free_cus -- the FM side stream's kernels avoid this many compute units (a CU-masked
    # stream, afm_stream_create_cu_mask), so the latency-bound tail beside the FM MFMA Grams keeps
    # whole CUs; 0 = an ordinary stream
    fm_free_cus: int = 0
    # fm_grid -- the FM per-date Grams' persistent workgroups (0: one per CU); an A/B knob
    fm_grid: int = 0
    # early_zstats -- the factor panel in two time slabs (afm_factors_range_f64): the train
    # window's z statistics run on a side stream while the second slab builds (a shard's factor
    # kernel leaves most of the GPU free: one wave per job set).  Measured at the N = 8 shard
    # (1,280 assets): 8.97 ms per step either way -- the second slab is the ~17 % of dates after
    # the train window, and the z statistics beside it ran 1.69 instead of 1.03 ms -- so off
    early_zstats: bool = False
    # zstats_slabs -- the factor panel in this many time slabs with the train window's z
    # statistics streamed slab by slab on a side stream right behind them (the recurrences' state
    # carried, afm_zscore_stats_slab_f64): on the smallest grids (the factor launch with one job
    # wave per SIMD, <= 25 blocks: the N = 8 shard) the z statistics then run on the issue slots
    # and CUs the factor kernel leaves free instead of after it.  -1: 6 on those grids, else 0.
    zstats_slabs: int = -1
    # early_fwd -- the analyzer's price rows and forward returns (prediction-independent,
    # KKT:294-296) on a side stream as soon as the all_df rows exist -- one GPU: beside the z
    # statistics; N > 1: after one all-gather of the all_df row words, beside the Grams --
    # instead of at the head of the analyzer stream in the tail
    early_fwd: bool = True
    # reb_split -- N > 1: each rank runs the rebalance of its share of the dates (+ one neighbour
    # per side) and one packed all-gather assembles the books; False: every rank runs every date
    # (the rebalance is latency-bound -- one workgroup per (date, side) -- so a rank's share is
    # not much shorter than all of it) and there is no exchange
    reb_split: bool = True


@dataclass
class Split:
    """The reference's date split on the calendar (KKT:424-428): ``.loc`` slices are inclusive at
    both ends.  train = [0, tr1), valid = [v0, v1), test = [s0, T); ``dup``: train_end is a
    trading date, so it is in train AND valid (its rows enter the fit twice)."""
    tr1: int
    v0: int
    v1: int
    s0: int
    dup: bool

    @classmethod
    def of(cls, dates, train_end, valid_end) -> "Split":
        d = np.asarray(dates).astype("datetime64[ns]")
        te = np.datetime64(np.datetime64(train_end, "D"), "ns")
        ve = np.datetime64(np.datetime64(valid_end, "D"), "ns")
        tr1 = int(np.searchsorted(d, te, side="right"))
        v0 = int(np.searchsorted(d, te, side="left"))
        v1 = int(np.searchsorted(d, ve, side="right"))
        s0 = int(np.searchsorted(d, ve, side="left"))
        if tr1 < 2 or s0 >= len(d) - 1 or v1 <= v0:
            raise ValueError(f"split {train_end} / {valid_end} leaves an empty train, valid or "
                             f"test range on {d[0]} .. {d[-1]}")
        return cls(tr1, v0, v1, s0, bool(v0 < tr1))


def block_assets(lda: int, nblk: int = N_BLOCKS) -> int:
    """Assets per Gram block: the 64-asset groups split into nblk equal runs."""
    return max(1, -(-(lda // 64) // nblk)) * 64


def _round_up(x: int, m: int = 64) -> int:
    return (x + m - 1) // m * m


def even_range(n: int, world: int, rank: int):
    """[lo, hi) of ``rank``'s share of ``n`` items split evenly over ``world`` ranks."""
    return n * rank // world, n * (rank + 1) // world


def _share_rows(ranges, stride: int, device):
    """Rows of the per-rank shares in an all-gathered [world][stride] buffer, in global order
    (rank q's i-th item at row q * stride + i): ONE index_select places every rank's share."""
    import torch
    return torch.as_tensor(np.concatenate([q * stride + np.arange(b - a) for q, (a, b)
                                           in enumerate(ranges)]).astype(np.int64), device=device)


class Pipeline:
    """The chain on one device, or on one rank of ``comm.world`` (``comm``: afm.sharded.Comm).

    Sharding (one process per GPU): rank r owns the asset blocks
    [8r/N, 8(r+1)/N) of the fixed 8-block split -- its factor panel, z-score statistics, pooled
    Gram partials (tree over its row-blocks and blocks) and per-date FM partials.  The
    exchanges: one all-gather of the block results of the pooled Gram (+ the train_end subtree),
    one all-gather of the test-date predictions and row bits, one all_to_all of per-date FM
    partials to the date owners (+ an all-gather of the betas), one all-gather of the rebalance
    results (rebalance dates are split over ranks).  Every sum follows the same fixed trees as
    one device, so every result is bit-identical to N = 1.

    Streams: a step runs on ``main``, side work forked onto ``side`` / ``side2`` / ``side3``.  Every
    switch of stream is a ``with self.ctx.on(stream):`` scope (torch's current stream and the afm
    context move and are restored together); every launch in it is a ``self.ctx.call``."""

    def __init__(self, grid: PanelGrid, cfg: PipelineConfig | None = None, comm=None):
        import torch
        self.full = grid
        self.comm = comm
        self.W = W = comm.world if comm is not None else 1
        self.rank = comm.rank if comm is not None else 0
        self.cfg = c = cfg or PipelineConfig()
        self.ctx = _lib.Context.get(grid.device.index)
        T, lda, A = grid.T, grid.lda, grid.A
        self.T, self.lda, self.A, self.nch = T, lda, A, (T + 63) // 64
        self.sp = Split.of(grid.dates, c.train_end, c.valid_end)
        self.features = list(c.features) if c.features is not None else FEATURES
        self.p, self.pf = len(self.features), len(c.fm_features)
        self.p2 = self.p + 2
        self.fwd_early = bool(c.analyzer and c.early_fwd)
        self.fm_at = c.fm_fork if W == 1 else "gram"     # N > 1: beside the lasso, always
        # tensor options (f64, i64, i32) on the panel's device
        self._opts = tuple(dict(dtype=t, device=grid.device)
                           for t in (torch.float64, torch.int64, torch.int32))
        self._init_shard()
        self._init_shard_buffers()
        self._init_fm_buffers()
        self._init_reb_buffers()
        self._init_analyzer_buffers()
        self._init_streams()
        self._init_slabs()
        self._stepped = False               # a step has filled the panel (factor_screen)
        self._screen_bufs = None

    def _init_shard(self):
        """The asset shard: whole blocks of the fixed split, and this rank's slice of the grid."""
        import torch
        grid, W, rk, A, lda = self.full, self.W, self.rank, self.A, self.lda
        if N_BLOCKS % W:
            raise ValueError(f"{W} ranks: the GPU count must divide {N_BLOCKS}")
        self.blk = blk = block_assets(lda)
        self.rb_per_blk = blk // 64
        if self.rb_per_blk > 32:          # the Gram trees merge at most 32 leaves a level
            raise ValueError(f"{A} assets: the pooled-Gram tree holds at most "
                             f"{N_BLOCKS * 32 * 64} assets ({N_BLOCKS} blocks x 32 row-blocks "
                             f"of 64)")
        self.nblk_r = N_BLOCKS // W
        self.wide = wide = self.nblk_r * blk           # padded shard width of the exchanges
        self.ranges = [(min(q * wide, A), min((q + 1) * wide, A)) for q in range(W)]
        a0, a1 = self.ranges[rk]
        self.a0, self.A_r = a0, a1 - a0
        self.lda_r = lda_r = _round_up(max(self.A_r, 1))
        self.nrb = (self.A_r + 63) // 64               # this shard's 64-asset row-blocks
        if W == 1:
            self.g = grid
        else:
            sl = slice(a0, a0 + lda_r)
            planes = ("close", "volume", "ret1d", "excess", "valid", "vbits")
            self.g = PanelGrid(dates=grid.dates, ids=grid.ids[a0:a1],
                               **{k: getattr(grid, k)[:, sl].contiguous() for k in planes})
        self.feat = torch.as_tensor(np.array([COL[n] for n in self.features], np.int32),
                                    device=grid.device)

    def _init_shard_buffers(self):
        """The shard's panel, row sets, z statistics, pooled-Gram partials and the fit."""
        import torch
        f64, i64, i32 = self._opts
        T, nch, lda_r, p, W, nrb = self.T, self.nch, self.lda_r, self.p, self.W, max(self.nrb, 1)
        self.out = torch.full((N_FACTORS, T, lda_r), float("nan"), **f64)
        self.nanfree = torch.zeros((nch, lda_r), **i64)
        self.finite = torch.zeros((nch, lda_r), **i64)
        self.alldf = torch.zeros((nch, lda_r), **i64)    # all_df rows (NT:33 dropna)
        self.frows = torch.zeros((nch, lda_r), **i64)    # all_df rows with every feature finite
        self.zrows = torch.zeros((nch, lda_r), **i64)    # rows surviving the z-score dropna
        self.mu = torch.empty((p, lda_r), **f64)
        self.sd = torch.empty((p, lda_r), **f64)
        self.zs = torch.empty((p + 1, lda_r, 2), **f64)
        self.asset_ok = torch.empty(lda_r, **i32)
        self.pe = pe = self.ctx.call("afm_zgram_part_bytes", p) // 8
        self.pool_part = torch.empty((nrb, N_CHUNKS, pe), **f64)
        self.pool_blk = torch.zeros((self.nblk_r + 1, pe), **f64)   # + the train_end subtree
        self.pool_all = torch.zeros((N_BLOCKS, pe), **f64)
        self.te_part = torch.zeros((self.nblk_r, pe), **f64)
        self.te_all = torch.zeros((W, pe), **f64)
        self.pool_g = torch.empty((1, self.p2, self.p2), **f64)
        self.pool_s = torch.zeros((1, self.p2), **f64)   # raw moments: zero shift
        self.te_gram = torch.zeros((1, self.p2, self.p2), **f64)
        self.lasso_beta = torch.empty(p + 1, **f64)
        self.lasso_info = torch.empty(3, **f64)

    def _init_fm_buffers(self):
        """FM design: [1, FM30 factor values, target] per date; the dates split over the ranks."""
        import torch
        f64, _, i32 = self._opts
        T, W, pf = self.T, self.W, self.pf
        self.fm_cols = torch.as_tensor(np.array([COL[n] for n in self.cfg.fm_features], np.int32),
                                       device=self.full.device)
        self.pef = pef = self.ctx.call("afm_zgram_part_bytes", pf) // 8
        self.fm_part = torch.zeros((T, self.nblk_r, pef), **f64)
        # this shard's subtree per date (N > 1: what the exchange sends; one GPU solves straight
        # from fm_part)
        self.fm_sub = torch.zeros((T if W > 1 else 0, pef), **f64)
        self.fdr = [even_range(T, W, q) for q in range(W)]   # FM dates owned by each rank
        fd0, fd1 = self.fdr[self.rank]
        self.fd0, self.fnd = fd0, fd1 - fd0
        self.fnd_max = max(b - a for a, b in self.fdr)
        self.fm_shift = torch.zeros((max(self.fnd, 1), pf + 2), **f64)
        self.fm_beta_own = torch.full((self.fnd_max, pf + 1), float("nan"), **f64)
        self.fm_nobs_own = torch.zeros(self.fnd_max, **f64)
        self.fm_rank_own = torch.zeros(self.fnd_max, **i32)
        if W == 1:
            self.fm_beta, self.fm_nobs, self.fm_rank = (self.fm_beta_own, self.fm_nobs_own,
                                                        self.fm_rank_own)
        else:
            self.fm_beta = torch.empty((T, pf + 1), **f64)
            self.fm_nobs = torch.empty(T, **f64)
            self.fm_rank = torch.empty(T, **i32)
        self.fm_mean = torch.empty(pf + 1, **f64)
        self.fm_t = torch.empty(pf + 1, **f64)

    def _init_reb_buffers(self):
        """The predictions, the full-width planes the rebalance / analyzer read, the rebalance
        dates (split over the ranks) with their books, and the PnL series."""
        import torch
        f64, i64, i32 = self._opts
        grid, c, sp, W, rk = self.full, self.cfg, self.sp, self.W, self.rank
        T, lda, nch, dev = self.T, self.lda, self.nch, self.full.device
        self.pred_r = torch.full((T, self.lda_r), float("nan"), **f64)
        if W == 1:
            self.pred, self.zrows_full, self.alldf_full = self.pred_r, self.zrows, self.alldf
            self.target, self.tmr = self.out[TARGET], self.out[TMR]
        else:
            self.pred = torch.full((T, lda), float("nan"), **f64)
            self.zrows_full = torch.zeros((nch, lda), **i64)
            self.alldf_full = torch.zeros((nch, lda), **i64)
            self.target = torch.full((T, lda), float("nan"), **f64)
            self.tmr = torch.full((T, lda), float("nan"), **f64)
            self.lab0 = 0 if c.window is None else max(0, sp.s0 - int(c.window) - 1)
        # rebalance dates: the test dates that can carry predictions (a present observation that
        # is not the asset's last -- every other row lacks the target)
        vb = grid.valid.cpu().numpy()
        nxt = np.zeros_like(vb)
        nxt[:-1] = np.flip(np.logical_or.accumulate(np.flip(vb[1:], 0), 0), 0)
        has = (vb & nxt).any(axis=1)
        rd = np.flatnonzero(has[sp.s0:]).astype(np.int32) + sp.s0
        self.nd = nd = len(rd)

        def reb_buffers(n):
            n = max(n, 1)
            return {"k": torch.zeros(n, **i32),
                    "books": torch.full((n, 2, MAX_BOOK), -1, **i32),
                    "weights": torch.zeros((n, 2, MAX_BOOK), **f64),
                    "sums": torch.zeros((n, 4), **f64),
                    "upos": torch.full((n, 2, 2, MAX_BOOK), -1, **i32),
                    "usize": torch.zeros((n, 2), **i64),
                    "status": torch.zeros(n, **i32)}
        self.reb = reb_buffers(nd)
        # rebalance dates of this rank (+ one neighbour per side: the turnover alignment needs the
        # adjacent dates' prediction sets)
        self.reb_split = W > 1 and c.reb_split
        Wr = W if self.reb_split else 1
        self.rrange = [even_range(nd, Wr, q) for q in range(Wr)]
        self.i0, self.i1 = i0, i1 = self.rrange[rk if self.reb_split else 0]
        self.e0, self.e1 = (max(i0 - 1, 0), min(i1 + 1, nd)) if self.reb_split else (0, nd)
        self.rd_ext = torch.from_numpy(rd[self.e0:self.e1].copy()).to(dev)
        self.rdates = torch.from_numpy(rd).to(dev)
        self.reb_ext = reb_buffers(self.e1 - self.e0) if self.reb_split else self.reb
        self._rows = {}                     # cached row indices of the share gathers (N > 1)
        self._send = {}                     # packed send buffers of the exchanges (N > 1)
        self.pnl = {"value": torch.empty(nd + 1, **f64), "turnover": torch.empty(nd, **f64),
                    "long_ret": torch.empty(nd, **f64), "short_ret": torch.empty(nd, **f64)}

    def _init_analyzer_buffers(self):
        """The analyzer on the test sub-grid (64-date aligned, so the bit words line up)."""
        import torch
        f64, i64, i32 = self._opts
        grid, sp, W, T, lda, dev = self.full, self.sp, self.W, self.T, self.lda, self.full.device
        self.an_a0 = (sp.s0 // 64) * 64
        self.Ta = Ta = T - self.an_a0
        self.price_bits = torch.zeros((self.nch, lda), **i64)   # df_test rows (all_df, test dates)
        if not self.cfg.analyzer:
            return
        ad = np.arange(sp.s0 - self.an_a0, Ta, dtype=np.int32)   # test dates, sub-grid index
        self.an_dates = torch.from_numpy(ad).to(dev)
        self.an_nd = nad = len(ad)
        years = np.asarray(grid.dates).astype("datetime64[Y]").astype(np.int64) + 1970
        yr = years[self.an_a0 + ad].astype(np.int32)
        self.an_year0, self.an_nyears = int(yr.min()), int(yr.max() - yr.min() + 1)
        self.an_year = torch.from_numpy(yr).to(dev)
        self.an = {
            "fr": torch.empty((3, Ta, lda), **f64), "scratch": torch.empty((Ta, lda), **f64),
            "rows": torch.empty((4, Ta, lda), **f64), "rows_idx": torch.empty((Ta, lda), **i32),
            "nrows": torch.empty(Ta, **i32), "skey": torch.empty((Ta, lda), **i64),
            "sidx": torch.empty((Ta, lda), **i32), "ra": torch.empty((Ta, lda), **i32),
            "rd": torch.empty((Ta, lda), **i32), "ic": torch.empty((nad, 3), **f64),
            "layer_mean": torch.empty((nad, 3, 10), **f64),
            "layer_cnt": torch.empty((nad, 10), **i32), "port": torch.empty((nad, 3), **f64),
            "cum_layer": torch.empty((nad, 3, 10), **f64), "ls": torch.empty((nad, 3, 5), **f64),
            "cum_port": torch.empty((nad, 3), **f64),
            "ir": torch.empty((self.an_nyears, 3), **f64),
            "ir_scratch": torch.empty((3 * self.an_nyears, nad), **f64),
        }
        # N > 1: each rank evaluates an even share of the test dates (every stage of the
        # analyzer but the final series is per date); one packed all-gather of the per-date
        # results, then every rank runs the series
        self.an_ranges = [even_range(nad, W, q) for q in range(W)]
        self.an_rng = self.an_ranges[self.rank]

    def _init_streams(self):
        """The step's streams, created in the order main, side, side2, side3."""
        import torch
        c, W, dev = self.cfg, self.W, self.full.device
        if c.fm_fork not in ("pool", "gram", "predict", "analyzer", "rebalance"):
            raise ValueError(f"fm_fork={c.fm_fork!r}: expected pool, gram, predict, analyzer or "
                             "rebalance")
        self.ncu = torch.cuda.get_device_properties(dev).multi_processor_count
        self.main = torch.cuda.Stream(device=dev, priority=-8 if c.main_priority else 0)
        self.fm_grid = c.fm_grid          # the FM Grams' persistent grid (0: one per CU)
        if c.fm_free_cus > 0:
            self._side_owner = _lib.cu_mask_stream(dev.index, c.fm_free_cus)
            self.side = self._side_owner.stream
            # one workgroup per CU the masked stream may use: a full-width grid would run the
            # surplus workgroups in a second round
            self.fm_grid = self.ncu - c.fm_free_cus
        else:
            self.side = torch.cuda.Stream(device=dev, priority=0)
        self.side2 = torch.cuda.Stream(device=dev, priority=0)
        # N > 1: the sequential PnL scan on its own stream, beside the FM exchange / solve and the
        # analyzer's gather + series that follow the rebalance (they no longer wait for it).  One
        # GPU creates no fourth stream: HIP maps streams onto GPU_MAX_HW_QUEUES (4) hardware queues
        # in creation order, and a stream that shares a queue waits behind the other's kernels
        self.side3 = (torch.cuda.Stream(device=dev, priority=-8 if c.main_priority else 0)
                      if W > 1 else self.main)
        self.streams = (self.main, self.side, self.side2) + ((self.side3,) if W > 1 else ())
        self.labels_done = torch.cuda.Event()

    def _init_slabs(self):
        """The time slabs of the streamed / early factor stages: bounds, carried state, events."""
        import torch
        f64, i64, _ = self._opts
        c, sp, T, A_r, lda_r = self.cfg, self.sp, self.T, self.A_r, self.lda_r
        # early z statistics: the first slab ends at the first 64-date boundary past the train
        # window (the slab API's alignment)
        self.ta = min(((sp.tr1 + 63) // 64) * 64, T)
        nslab = c.zstats_slabs
        if nslab < 0:
            nslab = 6 if self.nrb * 10 <= self.ncu else 0
        self.stream_z = nslab >= 2 and A_r > 0 and sp.tr1 > 0 and T >= 128
        if self.stream_z:
            self.zbounds = bounds = sorted({0, T} | {min(T, ((i * T // nslab + 63) // 64) * 64)
                                                     for i in range(1, nslab)})
            self.zstate = torch.empty((5, self.p, lda_r), **f64)
            self.zparts = [torch.empty(self.ctx.call("afm_factors_part_words", A_r, lda_r, a, z),
                                       **i64) for a, z in zip(bounds[:-1], bounds[1:])]
            self.zslab_done = [torch.cuda.Event() for _ in bounds[:-1]]
        self.early = (bool(c.early_zstats) and not self.stream_z and A_r > 0 and self.ta < T)
        if self.early or self.stream_z:
            nb = self.ctx.call("afm_factors_state_bytes", A_r)
            self.fstate = torch.empty(nb // 8 + 1, **f64)
            self.slab1_done = torch.cuda.Event()
            self.zstats_done = torch.cuda.Event()

    @property
    def labels_in_factor_stage(self) -> bool:
        """The two label planes are written inside the ``factors`` stage (main stream) rather
        than on a side stream beside it: one GPU with ``labels_side`` off (bench.py's roofline
        counts their bytes against that stage only then)."""
        return self.W == 1 and not self.cfg.labels_side

    def n_asset_days_local(self) -> int:
        return int(self.g.valid.sum().item())

    # ---- launch runs shared by the stages ------------------------------------------------------
    def _labels(self, stream, full=False):
        """The two label planes on ``stream``, then ``labels_done``: this shard's planes of the
        panel, or (``full``, N > 1) the full-width planes the rebalance reads."""
        g, lda, t0, tgt, tmr = ((self.full, self.lda, self.lab0, self.target, self.tmr) if full
                                else (self.g, self.lda_r, 0, self.out[TARGET], self.out[TMR]))
        with self.ctx.on(stream):
            self.ctx.call("afm_labels_f64", self.T, lda, t0, self.T, g.excess, g.ret1d, g.vbits,
                          tgt, tmr)
            self.labels_done.record(stream)

    def _last_obs_rows(self, t0=None, t1=None):
        """nanfree -> all_df rows and finite -> frows (an asset's last observation dropped), of
        every date or of the dates [t0, t1)."""
        fn, rng = (("afm_drop_last_obs_bits", ()) if t0 is None
                   else ("afm_drop_last_obs_bits_range", (t0, t1)))
        for src, dst in ((self.nanfree, self.alldf), (self.finite, self.frows)):
            self.ctx.call(fn, self.T, self.lda_r, self.g.vbits, src, dst, *rng)

    def _zrows(self, w0, nw, nt):
        """The z-score rows (frows of the surviving assets) of the ``nw`` 64-date words from
        ``w0`` on, ``nt`` dates."""
        self.ctx.call("afm_row_bits", nw, self.lda_r, self.frows[w0:], None, self.asset_ok, 0, nt,
                      self.zrows[w0:])

    def _zstats(self, nw, nt):
        """The train window's z statistics, the surviving assets, and the z-score rows of the
        first ``nw`` words (``nt`` dates)."""
        call, T, lda_r, p = self.ctx.call, self.T, self.lda_r, self.p
        call("afm_zscore_stats_f64", self.out, T * lda_r, T, lda_r, self.feat, p, self.alldf, 0,
             self.sp.tr1, self.mu, self.sd)
        call("afm_zstats_rows_f64", self.mu, self.sd, p, lda_r, self.zs, self.asset_ok, nw,
             self.frows, 0, nt, self.zrows)

    def _pooled_blocks(self, t0, nt, bufs=None, mark=None, after_pool=None):
        """This shard's pooled-Gram block results (rows of the dates [t0, t0 + nt)): row-block x
        chunk partials, then the tree in one launch -- the chunks of a row-block (32, then 2), the
        row-blocks of an asset block -> pool_blk[0:nblk_r] (every block written: zeros where the
        shard has no row-block), or in the buffers ``bufs`` (part, blk) instead of the step's.
        ``after_pool()`` runs between the partial kernel's launch and the tree's."""
        call, T, lda, p = self.ctx.call, self.T, self.lda_r, self.p
        part, blk = bufs or (self.pool_part, self.pool_blk)
        if self.nrb == 0:
            blk[:self.nblk_r].zero_()
            if after_pool is not None:
                after_pool()
            return
        if mark is not None:
            mark("k_gram", 0)
        call("afm_zpool_f64", self.out, T * lda, lda, self.feat, None, p, TARGET, self.zs, p,
             self.zrows, t0, nt, 0, self.nrb, self.A_r, N_CHUNKS, part, 0)
        if mark is not None:
            mark("k_gram", 1)
        if after_pool is not None:
            after_pool()
        c1, c2 = CHUNK_TREE
        call("afm_gram_tree3_f64", p, part, self.nrb, c1, c2, self.rb_per_blk, self.nblk_r, blk)

    def _te_subtree(self, t):
        """This shard's block partials of the train_end date's Gram -> te_part; N > 1: their
        subtree -> pool_blk[nblk_r] (what the exchange sends; one GPU merges the block partials
        in the final launch: the tree over its 8 leaves is the subtree, then a one-leaf level)."""
        call, T, lda, p = self.ctx.call, self.T, self.lda_r, self.p
        if self.nrb == 0:
            return
        call("afm_zgram_f64", self.out, T * lda, lda, self.feat, None, p, TARGET, self.zs, p,
             self.zrows, t, 1, self.nblk_r, 0, self.blk, self.A_r, self.te_part, 0)
        if self.W > 1:
            call("afm_gram_tree_f64", p, self.te_part, self.nblk_r, self.nblk_r, 0,
                 self.pool_blk[self.nblk_r:])

    def _fm_local(self):
        """This shard's per-date FM30 partials over the z-score rows -> fm_part [T][nblk_r];
        N > 1: merged over its blocks -> fm_sub [T]."""
        call, T, lda, pf = self.ctx.call, self.T, self.lda_r, self.pf
        if self.nrb == 0:
            return
        call("afm_zgram_f64", self.out, T * lda, lda, self.fm_cols, None, pf, TARGET, None, 0,
             self.zrows, 0, T, self.nblk_r, 0, self.blk, self.A_r, self.fm_part, self.fm_grid)
        if self.W > 1:
            call("afm_gram_tree_f64", pf, self.fm_part, T * self.nblk_r, self.nblk_r, 0,
                 self.fm_sub)

    def _fm_solve(self, leaves, per):
        """Owned dates: each date's ``per`` partials ``leaves`` [fnd][per][part] merged over the
        fixed tree while the solve loads them -- N > 1: the W rank subtrees; one GPU: the block
        partials themselves (the tree over the 8 blocks, then a one-leaf level)."""
        if self.fnd > 0:
            self.ctx.call("afm_ols_solve_parts_f64", leaves, per, self.fm_shift, self.pf, self.fnd,
                          self.cfg.tol, self.fm_beta_own, self.fm_nobs_own, self.fm_rank_own)

    def _fm_stats(self):
        self.ctx.call("afm_fama_macbeth_f64", self.fm_beta, self.fm_rank, self.T, self.pf + 1,
                      self.fm_mean, self.fm_t)

    # ---- the factor stage's three paths --------------------------------------------------------
    def _factors_one_pass(self, lab_side, mark):
        """The factor panel and the all_df rows in one call on the main stream.  One GPU: the
        two label planes on the second side stream, enqueued after the factor kernel (it runs
        on the CUs the factor workgroups leave free); the z statistics wait for them."""
        g = self.g
        if self.A_r > 0:
            mark("k_factor", 0)
            self.ctx.call("afm_factors_rows_f64", self.T, self.A_r, self.lda_r, g.close, g.volume,
                          None if lab_side else g.ret1d, None if lab_side else g.excess, g.vbits,
                          self.out, self.nanfree, self.finite, self.alldf, self.frows)
            mark("k_factor", 1)
            if lab_side:
                self._labels(self.side2)
        mark("factors", 1)

    def _factors_streamed(self, lab_side, mark):
        """The factor panel in time slabs (zbounds) on the main stream, each slab's all_df rows
        right behind it, and the train window's z statistics streamed slab by slab on the side
        stream as each slab lands (afm_zscore_stats_slab_f64, every (feature, asset) recurrence
        carried): bitwise the panel, statistics and row sets of one call each.  The label planes
        go first, once, on the second side stream (inputs only; tmr_ret1d is a feature) -- not
        inside every factor slab; with ``labels_side`` off, on the main stream ahead of the first
        slab, inside the factors stage)."""
        import torch
        call, g, T, lda_r, p, A_r = self.ctx.call, self.g, self.T, self.lda_r, self.p, self.A_r
        self._labels(self.side2 if lab_side else self.main)
        b, tr1 = self.zbounds, self.sp.tr1
        for i in range(len(b) - 1):
            t0, t1 = b[i], b[i + 1]
            # the slab on the main stream; its row masks, all_df rows and z statistics on the side
            # stream beside the next slab (the next slab needs only the carried factor state)
            need = call("afm_factors_part_words", A_r, lda_r, t0, t1)
            if need > self.zparts[i].numel():    # (an execution option changed the launch shape)
                self.zparts[i] = torch.empty(need, dtype=torch.int64, device=self.out.device)
            part = self.zparts[i]
            call("afm_factors_range_part_f64", T, A_r, lda_r, t0, t1, g.close, g.volume, g.vbits,
                 self.out, self.fstate, part)
            self.zslab_done[i].record(self.main)
            with self.ctx.on(self.side):
                self.side.wait_event(self.zslab_done[i])
                call("afm_factor_masks_f64", T, A_r, lda_r, t0, t1, g.vbits, part, self.nanfree,
                     self.finite)
                self._last_obs_rows(t0, t1)
                if t0 < tr1:
                    if i == 0:
                        self.side.wait_event(self.labels_done)
                        mark("zstats", 0)
                    last = t1 >= tr1
                    call("afm_zscore_stats_slab_f64", self.out, T * lda_r, T, lda_r, self.feat, p,
                         self.alldf, t0, min(t1, tr1), self.zstate, int(i == 0), int(last),
                         self.mu, self.sd)
                    if last:
                        call("afm_zstats_finalize_f64", self.mu, self.sd, p, lda_r, self.zs,
                             self.asset_ok)
                        mark("zstats", 1)
        mark("factors", 1)
        self.zstats_done.record(self.side)        # every slab's masks, rows and statistics
        self.main.wait_event(self.zstats_done)
        self._zrows(0, self.nch, T)

    def _factors_early(self, lab_side, mark):
        """The factor panel in two slabs [0, ta) and [ta, T) on the main stream; the train
        window's z statistics (and the z-score row bits of the first slab) on the side stream
        beside the second slab.  Bitwise the same panel, statistics and row sets as one call."""
        g, T, ta, wa = self.g, self.T, self.ta, self.ta // 64
        lab = (None, None) if lab_side else (g.ret1d, g.excess)

        def slab(t0, t1):
            self.ctx.call("afm_factors_range_f64", T, self.A_r, self.lda_r, t0, t1, g.close,
                          g.volume, *lab, g.vbits, self.out, self.nanfree, self.finite,
                          self.fstate)
        slab(0, ta)
        if lab_side:
            self._labels(self.side2)
        self._last_obs_rows(0, ta)
        self.slab1_done.record(self.main)
        with self.ctx.on(self.side):
            self.side.wait_event(self.slab1_done)
            if lab_side:
                self.side.wait_event(self.labels_done)          # tmr_ret1d is a feature
            mark("zstats", 0)
            self._zstats(wa, ta)
            mark("zstats", 1)
            self.zstats_done.record(self.side)
        slab(ta, T)
        self._last_obs_rows(ta, T)
        mark("factors", 1)
        self.main.wait_event(self.zstats_done)
        self._zrows(wa, self.nch - wa, T - ta)

    # ---- the step ------------------------------------------------------------------------------
    def step(self, events: dict | None = None):
        """One pass of the chain.  ``events``: optional {stage: (start, end)} CUDA events."""
        import torch
        caller = torch.cuda.current_stream(self.full.device)
        for s in self.streams:
            s.wait_stream(caller)

        def mark(stage, which):
            if events is not None and stage in events:
                events[stage][which].record()

        with self.ctx.on(self.main):
            self._stage_factors(mark)
            self._stage_gram(mark)
            self._stage_fit_predict(mark)
            self._stage_tail(mark)
        for s in self.streams:
            caller.wait_stream(s)
        self._stepped = True

    def _stage_factors(self, mark):
        """factors + zstats: the panel, the row sets and the train window's z statistics; the
        prediction-independent side work (label planes, the analyzer's forward returns) forked."""
        W, one_pass = self.W, not (self.early or self.stream_z)
        lab_side = W == 1 and self.cfg.labels_side
        mark("factors", 0)
        if self.stream_z:
            self._factors_streamed(lab_side, mark)
        elif self.early:
            self._factors_early(lab_side, mark)
        else:
            self._factors_one_pass(lab_side, mark)
        if self.fwd_early and W == 1:
            self.side2.wait_stream(self.main)                # the all_df rows
            with self.ctx.on(self.side2):
                self._analyzer_fwd()
        if one_pass:
            mark("zstats", 0)
            if self.A_r > 0:
                if lab_side:
                    self.main.wait_event(self.labels_done)          # tmr_ret1d is a feature
                self._zstats(self.nch, self.T)
            mark("zstats", 1)
        if W > 1:           # full-width label planes for the rebalance, during the Grams
            self._labels(self.side2, full=True)
            if self.fwd_early:
                # the analyzer's price rows and forward returns need the whole cross-section's
                # all_df rows only (not the predictions): gathered now, beside the Grams, so
                # the analyzer's prediction-dependent chain starts right at the predict
                self.side2.wait_stream(self.main)            # the all_df rows (after zstats)
                with self.ctx.on(self.side2):
                    self._gather_alldf()
                    self._analyzer_fwd()

    def _stage_gram(self, mark):
        """xs_gram: the pooled Gram of the train + valid rows (block results, N > 1: exchanged,
        then the block level of the tree), train_end's Gram added once more."""
        call, sp, p, W = self.ctx.call, self.sp, self.p, self.W
        mark("xs_gram", 0)
        # train_end counted twice: its Gram first (it needs the z statistics and rows only), so
        # that no kernel with a whole CU's LDS follows the pooled kernel and the FM Grams, which
        # cannot share a CU with it, may start there
        if sp.dup:
            self._te_subtree(sp.tr1 - 1)
        self._pooled_blocks(0, sp.v1, mark=mark,                # train + valid rows
                            after_pool=lambda: self._fork_fm("pool", mark))
        if W > 1:
            mark("exchange", 0)
            gb = self.comm.all_gather(self.pool_blk)            # [W][nblk_r + 1][part]
            self.pool_all.copy_(gb[:, :self.nblk_r].reshape(N_BLOCKS, self.pe))
            self.te_all.copy_(gb[:, self.nblk_r])
            mark("exchange", 1)
            blocks, te_leaves, nte = self.pool_all, self.te_all, W
        else:
            blocks, te_leaves, nte = self.pool_blk, self.te_part, self.nblk_r
        call("afm_gram_final_f64", p, blocks, N_BLOCKS, te_leaves if sp.dup else None, nte,
             self.pool_g, self.te_gram)
        mark("xs_gram", 1)

    def _fork_fm(self, at, mark):
        """Side stream, if the FM fork point is ``at``: this shard's per-date FM30 partials
        (nothing downstream reads them), forked after the pooled Gram -- run beside it, both MFMA
        kernels slow down (A/B on MI355X: pooled Gram 12.7 ms alone, 23 ms beside the FM Grams).
        One GPU: forked after the predict, ahead of the analyzer (A/B over 5 runs: 35.29 vs
        35.40 ms/step forked after the Gram; 36.4-37.0 after the analyzer, 36.5-36.7 after the
        rebalance); ``PipelineConfig.fm_fork`` moves it."""
        if at != self.fm_at:
            return
        self.side.wait_stream(self.main)
        with self.ctx.on(self.side):
            mark("fm", 0)
            self._fm_local()
            if self.W == 1:
                self._fm_solve(self.fm_part, self.nblk_r)
                self._fm_stats()
            mark("fm", 1)

    def _stage_fit_predict(self, mark):
        """lasso + predict (N > 1: the test dates' whole cross-section gathered)."""
        call, c, sp, T, lda_r, p = self.ctx.call, self.cfg, self.sp, self.T, self.lda_r, self.p
        self._fork_fm("gram", mark)
        mark("lasso", 0)
        call("afm_lasso_fit_f64", self.pool_g, self.pool_s, p, c.alpha, c.max_iter, c.lasso_tol,
             0, self.lasso_beta, self.lasso_info)
        mark("lasso", 1)
        mark("predict", 0)
        if self.A_r > 0:
            call("afm_zpredict_f64", self.out, T * lda_r, lda_r, sp.s0, T - sp.s0, self.feat, p,
                 self.zs, self.lasso_beta, self.zrows, self.pred_r)
        if self.W > 1:                          # the whole cross-section of the test dates
            self._gather_test_planes()
        mark("predict", 1)
        self._fork_fm("predict", mark)

    def _stage_tail(self, mark):
        """The analyzer forked onto the second side stream; rebalance and pnl on the main stream;
        N > 1: the scan on its own stream beside the FM exchange and the analyzer's series."""
        c, sp, full, W = self.cfg, self.sp, self.full, self.W
        if c.analyzer:
            self.side2.wait_stream(self.main)
            with self.ctx.on(self.side2):
                self._analyzer(mark)
        self._fork_fm("analyzer", mark)
        mark("rebalance", 0)
        if W > 1:
            self.main.wait_event(self.labels_done)     # the label planes
        x, ne = self.reb_ext, self.e1 - self.e0
        if ne > 0 and c.risk_tolerance != 0:
            if c.expected not in ("prediction", "history"):
                raise ValueError(f"expected={c.expected!r}: expected prediction or history")
            self.ctx.call("afm_rebalance_mv_f64", self.T, full.A, full.lda, self.rd_ext, ne,
                          self.pred, full.tbits, self.target, self.zrows_full, 0, sp.tr1,
                          -1 if c.window is None else int(c.window), full.close, self.tmr,
                          c.top_n, c.lo, c.hi, self.pred if c.expected == "prediction" else None,
                          c.risk_tolerance, x["k"], x["books"], x["weights"], x["sums"],
                          x["upos"], x["usize"], x["status"])
        elif ne > 0:
            self.ctx.call("afm_rebalance_f64", self.T, full.A, full.lda, self.rd_ext, ne,
                          self.pred, full.tbits, self.target, self.zrows_full, 0, sp.tr1,
                          -1 if c.window is None else int(c.window), full.close, self.tmr,
                          c.top_n, c.lo, c.hi, x["k"], x["books"], x["weights"], x["sums"],
                          x["upos"], x["usize"], x["status"])
        if self.reb_split:
            self._gather_rebalance()
        mark("rebalance", 1)
        self._fork_fm("rebalance", mark)
        if W == 1:
            self._pnl_scan(mark)
            return
        # the scan on its own stream; the FM exchange (per-date subtrees -> date owners, solves,
        # betas) and the analyzer's gather + series run beside it on the main and second side
        # streams, issued in this order on every rank (RCCL runs a group's collectives in issue
        # order)
        self.side3.wait_stream(self.main)
        with self.ctx.on(self.side3):
            self._pnl_scan(mark)
        self.main.wait_stream(self.side)
        self._fm_exchange()
        if c.analyzer:
            with self.ctx.on(self.side2):
                self._analyzer_series(mark)

    def _pnl_scan(self, mark):
        c, r, q = self.cfg, self.reb, self.pnl
        mark("pnl", 0)
        self.ctx.call("afm_pnl_scan_f64", self.nd, r["k"], r["books"], r["sums"], r["upos"],
                      r["usize"], c.v0, c.rate, q["value"], q["turnover"], q["long_ret"],
                      q["short_ret"])
        mark("pnl", 1)

    # ---- exchanges (N > 1; a collective runs on the current stream and leaves the binding) ----
    def _send_buffer(self, key, specs, device):
        """The persistent packed send buffer of one exchange (made on its first step)."""
        from .packing import SendBuffer
        sb = self._send.get(key)
        if sb is None:
            sb = self._send[key] = SendBuffer(specs, device)
        return sb

    def _place_shares(self, key, ranges, gathered, dsts):
        """All-gathered date shares ``gathered[i]`` [W][largest share][...] -> ``dsts[i]`` in
        global order: ONE index_select per array (the row index cached under ``key``), not one
        copy per rank."""
        import torch
        rows = self._rows.get(key)
        if rows is None:                    # gathered row (rank q, i) of every date
            rows = self._rows[key] = _share_rows(ranges, gathered[0].shape[1],
                                                 gathered[0].device)
        if rows.numel():
            for g, dst in zip(gathered, dsts):
                torch.index_select(g.reshape((-1,) + tuple(g.shape[2:])), 0, rows, out=dst)

    def _gather_shares(self, key, srcs, own, ranges, dsts):
        """This rank's share (rows ``own[0]:own[1]``) of every array of ``srcs``, padded to the
        largest share, in one packed all-gather -> every rank's share placed in ``dsts``."""
        n = max(b - a for a, b in ranges)
        sb = self._send_buffer(key, [((n,) + tuple(v.shape[1:]), v.dtype, 0) for v in srcs],
                               srcs[0].device)
        for v, part in zip(srcs, sb.parts):          # rows past the share stay zero
            part[:own[1] - own[0]].copy_(v[own[0]:own[1]])
        self._place_shares(key, ranges, self.comm.all_gather_buffer(sb), dsts)

    def _gather_analyzer(self):
        """The per-date analyzer results of every rank's date share -> the full arrays."""
        srcs = [self.an[k] for k in ("ic", "layer_mean", "layer_cnt", "port")]
        self._gather_shares("an", srcs, self.an_rng, self.an_ranges,
                            [v[:self.an_nd] for v in srcs])

    def _gather_rebalance(self):
        """The books of every rank's share of the rebalance dates -> ``reb``."""
        lo = self.i0 - self.e0
        self._gather_shares("reb", list(self.reb_ext.values()), (lo, lo + self.i1 - self.i0),
                            self.rrange, [v[:self.nd] for v in self.reb.values()])

    def _place(self, dst, gathered, rows=None):
        """Scatter per-rank shard columns ([W][rows][wide]) into a full-width plane.  Rank q's
        columns start at q * wide (the fixed block split), so the ranks side by side ARE the
        plane's first W * wide columns: the full-width ranks in ONE strided copy straight into the
        plane (no reordered intermediate), the last (short) rank in a second -- not one copy per
        rank (each small copy is a launch the step waits on).  Columns from A on are untouched."""
        A = self.ranges[-1][1]
        if A == 0:
            return
        W, nr, wide = gathered.shape[0], gathered.shape[1], gathered.shape[2]
        d = dst if rows is None else dst[rows]
        k = (W - 1) * wide                  # the full-width ranks' columns
        if k <= A and A - k <= wide:
            if W > 1:
                d[:, :k].view(nr, W - 1, wide).copy_(gathered[:W - 1].permute(1, 0, 2))
            d[:, k:A] = gathered[W - 1, :, :A - k]
            return
        side = gathered.permute(1, 0, 2).reshape(nr, W * wide)
        d[:, :A] = side[:, :A]

    def _gather_test_planes(self):
        """The test dates' predictions and the z-score / all_df row words of every rank's asset
        shard -> the full-width planes (one packed all-gather; the all_df words already went
        out with the forward returns when those run early, ``_gather_alldf``)."""
        import torch
        s0, wide, A_r = self.sp.s0, self.wide, self.A_r
        specs = [((self.T - s0, wide), torch.float64, float("nan")),
                 ((self.nch, wide), torch.int64, 0)]
        with_alldf = not self.fwd_early
        if with_alldf:
            specs.append(((self.nch, wide), torch.int64, 0))
        sb = self._send_buffer("test" if with_alldf else "test_noad", specs, self.pred_r.device)
        pr, zb = sb.parts[:2]                       # columns past A_r keep NaN / 0
        if A_r > 0:
            pr[:, :A_r].copy_(self.pred_r[s0:, :A_r])
            zb[:, :A_r].copy_(self.zrows[:, :A_r])
            if with_alldf:
                sb.parts[2][:, :A_r].copy_(self.alldf[:, :A_r])
        got = self.comm.all_gather_buffer(sb)
        self._place(self.pred, got[0], rows=slice(s0, self.T))
        self._place(self.zrows_full, got[1])
        if with_alldf:
            self._place(self.alldf_full, got[2])

    def _gather_alldf(self):
        """Every rank's all_df row words -> the full-width ``alldf_full`` (one all-gather)."""
        import torch
        sb = self._send_buffer("alldf", [((self.nch, self.wide), torch.int64, 0)],
                               self.alldf.device)
        if self.A_r > 0:
            sb.parts[0][:, :self.A_r].copy_(self.alldf[:, :self.A_r])
        self._place(self.alldf_full, self.comm.all_gather_buffer(sb)[0])

    def _fm_exchange(self):
        """The per-date subtrees to the date owners (one all_to_all), their solves, then every
        rank gets every date's betas (one packed all-gather) and the FM statistics."""
        W = self.W
        recv = self.comm.all_to_all(self.fm_sub, [b - a for a, b in self.fdr],
                                    [self.fnd] * W)                          # [W * fnd][part]
        sub = recv.view(W, self.fnd, self.pef).transpose(0, 1).contiguous()   # [fnd][W][part]
        self._fm_solve(sub, W)
        got = self.comm.all_gather_packed([self.fm_beta_own, self.fm_nobs_own, self.fm_rank_own])
        self._place_shares("fm", self.fdr, got, (self.fm_beta, self.fm_nobs, self.fm_rank))
        self._fm_stats()

    # ---- the analyzer (second side stream) ------------------------------------------------------
    def _analyzer(self, mark):
        """AlphaSignalAnalyzer(lasso_predict, price_data=df_test[['close_price']]).run()
        (KKT:630-631) on the test sub-grid, no host synchronisation."""
        call, full, sp, an = self.ctx.call, self.full, self.sp, self.an
        lda, a0, Ta = full.lda, self.an_a0, self.Ta
        mark("analyzer", 0)
        if not self.fwd_early:
            self._analyzer_fwd()
        j0, j1 = self.an_rng
        d0 = sp.s0 - a0 + j0                        # sub-grid dates [d0, d1) of this rank
        d1 = d0 + (j1 - j0)
        if j1 > j0:
            call("afm_xs_prepare_range_f64", Ta, full.A, lda, d0, d1, self.pred[a0:], an["fr"],
                 an["scratch"], an["rows"], an["rows_idx"], an["nrows"])
            call("afm_xs_layers_f64", d1 - d0, lda, an["rows"][0, d0:], an["nrows"][d0:],
                 an["skey"][d0:], an["sidx"][d0:], an["ra"][d0:], an["rd"][d0:])
            call("afm_xs_stats_f64", Ta, lda, self.an_dates[j0:], j1 - j0, an["rows"],
                 an["nrows"], an["ra"], an["rd"], 10, an["ic"][j0:], an["layer_mean"][j0:],
                 an["layer_cnt"][j0:], an["port"][j0:])
        if self.W > 1:
            return          # the all-gather and the series follow the main chain's exchanges
        self._analyzer_series(mark)

    def _analyzer_fwd(self):
        """The analyzer's df_test price rows and forward returns (KKT:294-296): they read the close
        plane and the all_df rows only, not the predictions."""
        call, full, sp, a0 = self.ctx.call, self.full, self.sp, self.an_a0
        call("afm_row_bits", self.nch, full.lda, self.alldf_full, None, None, sp.s0, self.T,
             self.price_bits)
        call("afm_fwd_returns_f64", self.Ta, full.lda, full.close[a0:],
             self.price_bits[a0 // 64:], self.an["fr"])

    def _analyzer_series(self, mark):
        an = self.an
        if self.W > 1:
            self._gather_analyzer()
        self.ctx.call("afm_xs_series_f64", self.an_nd, an["layer_mean"], an["port"], an["ic"],
                      self.an_year, self.an_nyears, self.an_year0, an["cum_layer"], an["ls"],
                      an["cum_port"], an["ir"], an["ir_scratch"])
        mark("analyzer", 1)

    def _range_gram(self, t0, nt, bufs, gram):
        """The pooled Gram of the z-score rows of the dates [t0, t0 + nt) -> gram [1][p+2][p+2]:
        ``_pooled_blocks`` in the buffers ``bufs`` (not the step's) + the block level."""
        self._pooled_blocks(t0, nt, bufs)
        self.ctx.call("afm_gram_final_f64", self.p, bufs[1], N_BLOCKS, None, 0, gram, None)

    def lasso_cv(self, alphas=None, *, n_alphas: int = 100, eps: float = 1e-3) -> dict:
        """Validation-scored alpha selection on the last ``step()``'s panel (one GPU): the
        reference carries a ``valid`` split its linear models never use (KKT:426-427) and fixes
        alpha = 2e-4 (KKT:605).  The z statistics stay the train window's (KKT:449-454).

        The pooled Grams of train [0, tr1) and valid [v0, v1) are built like the step's (buffers
        of this call's own); the train Gram walks the alpha grid warm-started in one
        ``afm_lasso_batch_f64`` launch (``alphas``: descending after sorting; None: scikit-learn's
        grid of ``n_alphas`` from alpha_max down to ``eps`` alpha_max, on the train Gram); every
        model is scored on the valid Gram's moments (``afm_gram_score_f64``); the refit at the
        alpha of least valid MSE runs on the step's train+valid Gram (``pool_g``, train_end
        counted twice where the reference does).  Returns host arrays: ``alphas``, ``coefs``
        [n_alphas][p+1] (intercept first), ``n_iter``, ``dual_gap``, ``n_train``, ``n_valid``,
        ``mse_valid``, ``r2_valid``, ``ic_valid``, ``best``, ``alpha_``, ``beta`` (the refit)."""
        import torch
        from .regression import _given_alphas, alpha_grid, gram_score, lasso_batch
        if self.W > 1:
            raise NotImplementedError("lasso_cv() runs on one GPU (world = 1)")
        if self.nrb == 0:
            raise ValueError("lasso_cv(): the panel has no assets")
        c, sp, p = self.cfg, self.sp, self.p
        if getattr(self, "_cv_bufs", None) is None:
            self._cv_bufs = tuple(torch.empty_like(b) for b in (self.pool_part, self.pool_blk))
            self._cv_gram = torch.empty((2, self.p2, self.p2), dtype=torch.float64,
                                        device=self.out.device)
        gram, shift = self._cv_gram, self.pool_s.expand(2, self.p2).contiguous()
        with self.ctx.on(torch.cuda.current_stream(self.out.device)):        # the caller's stream
            self._range_gram(0, sp.tr1, self._cv_bufs, gram[0:1])
            self._range_gram(sp.v0, sp.v1 - sp.v0, self._cv_bufs, gram[1:2])
            a = _given_alphas(alphas) if alphas is not None else \
                alpha_grid(gram[0].cpu().numpy(), p, eps, n_alphas)
            beta, info = lasso_batch(gram[0:1], shift[0:1], p, torch.from_numpy(a).to(gram.device),
                                     nprob=1, warm=True, max_iter=c.max_iter, tol=c.lasso_tol)
            score = gram_score(gram[1:2], shift[1:2], p, beta).cpu().numpy()[0]
            n_train = float(gram[0, 0, 0].item())
            best = int(np.argmin(score[:, 1]))
            refit = torch.empty(p + 1, dtype=torch.float64, device=gram.device)
            rinfo = torch.empty(3, dtype=torch.float64, device=gram.device)
            self.ctx.call("afm_lasso_fit_f64", self.pool_g, self.pool_s, p, float(a[best]),
                          c.max_iter, c.lasso_tol, 0, refit, rinfo)
        info_h = info[0].cpu().numpy()
        return {"alphas": a, "coefs": beta[0].cpu().numpy(),
                "n_iter": info_h[:, 2].astype(np.int64), "dual_gap": info_h[:, 0] / n_train,
                "n_train": int(n_train), "n_valid": int(score[0, 0]),
                "mse_valid": score[:, 1].copy(), "r2_valid": score[:, 2].copy(),
                "ic_valid": score[:, 3].copy(), "best": best, "alpha_": float(a[best]),
                "beta": refit.cpu().numpy()}

    def factor_screen(self, split: str = "train", z: bool = True, columns=None,
                      corr_method: str = "pearson", layers: bool = False,
                      xcorr: bool = False, prep=None, groups=None, combine=None,
                      turnover=None) -> dict:
        """Factor screening on the last ``step()``'s resident panel (one GPU): the per-date IC
        (``corr_method``: 'pearson', or 'spearman' for the rank IC) of every column against
        return_1 / 2 / 5, its per-year IR and whole-sample
        summary (``afm.screen.screen_grid``) -- the reference's single-factor evaluation on a
        split (KKT:465, 472), all columns in one pass, before anything is fitted.

        ``split``: "train", "valid" or "test", the reference's inclusive date ranges (``Split``).
        ``z=True``: the rows are the z-score rows of the split's dates and the values are z on the
        fly from the train window's statistics (``df_train_x``); ``z=False``: the all_df rows and
        the raw values.  The price rows are the all_df rows of the split's dates (``price_data =
        df_train[['close_price']]``): forward returns do not look past the split.  ``columns``:
        factor names (default: the pipeline's features; with ``z`` they must be features).

        Runs on the caller's stream in buffers of its own (allocated on first use).  Returns host
        arrays ``ic`` [nd][K][3], ``stats`` [K][3][5] (n, mean, std, IR, t), ``ir_year``
        [nyears][K][3], ``nrows`` [T], ``dates_idx`` (calendar indices of the evaluated dates),
        ``years``, ``year0`` and the names ``features``.  ``layers=True``: also the decile layered
        returns, long-short spreads and top-10 backtest of every column on the same rows and dates
        (KKT:324-375) -- ``layer_mean`` [nd][K][3][10], ``layer_cnt`` [nd][K][10], ``port``
        [nd][K][3], ``cum_layer`` [nd][K][3][10], ``ls`` [nd][K][3][5], ``cum_port`` [nd][K][3],
        ``screen_grid``'s.

        ``xcorr=True``: also how the columns relate to each other (always Pearson) --
        ``xcorr_stats`` [K][K][3] = (n, mean r, mean \|r\|) over the dates of the per-date
        correlation matrix of the columns on the same rows, a host array; the per-date matrices
        ``xcorr_dev`` [nd][K][K] stay on the device (hundreds of MB at full size; the buffer is
        reused by the next call).  The intended loop -- screen, prune what is redundant, refit::

            r = pipe.factor_screen("train", xcorr=True)
            sel = select_factors(r["features"], r["stats"][:, 0, 3], r["xcorr_stats"][:, :, 2],
                                 max_corr=0.7, k=30)
            pipe2 = Pipeline(panel, PipelineConfig(fm_features=tuple(sel)))

        ``prep`` (an ``afm.xsprep.XsPrep``): every column is first winsorised / group-neutralised
        / standardised across each evaluated date, over the split's rows of that date (with ``z``
        the z values are what is preprocessed), and the screen reads the result
        (``screen_grid(..., prep=...)``).  ``groups``: a host array [A] of group (sector) labels of
        any dtype, one per security (default: the grid's ``group``; NaN: in no group).  The result
        gains ``prep_info`` [nd][K][7] = (n, lo, hi, n_lo, n_hi, mean, std).

        ``combine`` (an ``afm.combine.ICWeights``): the columns are combined into one signal, on
        every evaluated date weighted by their rolling ICs of the dates before it
        (``screen_grid(..., combine=...)``).  Host arrays ``weights`` [nd][K], ``weights_info``
        [nd][3], ``composite_ic`` [nd][3] and ``composite_stats`` [3][5]; the plane stays on the
        device as ``composite_dev`` [dates of the split's sub-grid][lda], whose row 0 is calendar
        date ``composite_t0`` (the buffer is reused by the next call).

        ``turnover`` (an ``afm.turnover.Turnover``): how much every column changes against the
        evaluated date ``lag`` positions earlier (``screen_grid(..., turnover=...)``).  Host arrays
        ``rank_ac`` [nd][K][L], ``turnover_counts`` [nd][K][L][5], ``port_turnover`` [nd][K][L] and
        ``turnover_stats`` [K][L][4][2]; with ``combine`` also the composite's, the names with
        ``composite_`` in front.

        Not the multi-GPU pipeline."""
        import torch
        from .analyzer import check_corr_method
        from .screen import screen_grid
        check_corr_method(corr_method)
        if self.W > 1:
            raise NotImplementedError("factor_screen() runs on one GPU (world = 1)")
        if not self._stepped:
            raise ValueError("factor_screen(): run step() first (the panel is empty)")
        sp, T, lda, nch, dev = self.sp, self.T, self.lda, self.nch, self.out.device
        try:
            t0, t1 = {"train": (0, sp.tr1), "valid": (sp.v0, sp.v1), "test": (sp.s0, T)}[split]
        except KeyError:
            raise ValueError(f"split={split!r}: expected train, valid or test") from None
        names = list(columns) if columns is not None else list(self.features)
        if z:
            missing = [n for n in names if n not in self.features]
            if missing:
                raise ValueError(f"factor_screen(z=True): {missing} are not features of this "
                                 "pipeline (no z statistics)")
        cols = np.array([COL[n] for n in names], np.int32)
        zcols = np.array([self.features.index(n) for n in names], np.int32) if z else None
        if self._screen_bufs is None:
            self._screen_bufs = {"row_bits": torch.zeros((nch, lda), **self._opts[1]),
                                 "price_bits": torch.zeros((nch, lda), **self._opts[1])}
        b = self._screen_bufs
        gdev, G = None, 0
        if prep is not None and prep.neutralize:
            from .xsprep import factorize_groups
            labels = groups if groups is not None else self.full.group
            if labels is None or len(labels) != self.A:
                raise ValueError("factor_screen(prep.neutralize): groups must hold one label per "
                                 f"security ({self.A})")
            codes, G = factorize_groups(labels)
            gdev = torch.full((lda,), -1, dtype=torch.int32, device=dev)
            gdev[:self.A] = torch.from_numpy(codes).to(dev)
        a0 = (t0 // 64) * 64                # the split's sub-grid, 64-date aligned (bit words)
        w0, w1 = a0 // 64, (t1 + 63) // 64
        years = np.asarray(self.full.dates).astype("datetime64[Y]").astype(np.int64) + 1970
        with self.ctx.on(torch.cuda.current_stream(dev)):                    # the caller's stream
            call = self.ctx.call
            call("afm_row_bits", nch, lda, self.zrows if z else self.alldf, None, None, t0, t1,
                 b["row_bits"])
            call("afm_row_bits", nch, lda, self.alldf, None, None, t0, t1, b["price_bits"])
            r = screen_grid(self.out[0, a0:t1], cols, self.full.close[a0:t1],
                            b["price_bits"][w0:w1], b["row_bits"][w0:w1], A=self.A,
                            zs=self.zs if z else None, zcols=zcols, col_stride=T * lda,
                            year=years[a0:t1], bufs=b, corr_method=corr_method,
                            layers=layers, xcorr=xcorr, prep=prep, groups=gdev,
                            ngroups=max(G, 1), combine=combine, turnover=turnover)
            keys = ("ic", "stats", "ir_year") + (("layer_mean", "layer_cnt", "port", "cum_layer",
                                                  "ls", "cum_port") if layers else ())
            if xcorr:
                keys += ("xcorr_stats",)
            if prep is not None:
                keys += ("prep_info",)
            if combine is not None:
                keys += ("weights", "weights_info", "composite_ic", "composite_stats")
            if turnover is not None:
                tk = ("rank_ac", "turnover_counts", "port_turnover", "turnover_stats")
                keys += tk + (tuple("composite_" + k for k in tk) if combine is not None else ())
            out = {k: r[k].cpu().numpy() for k in keys}
            if xcorr:
                out["xcorr_dev"] = r["xcorr"]
            if combine is not None:
                out["composite_dev"], out["composite_t0"] = r["composite"], a0
            nrows = np.zeros(T, dtype=np.int32)
            nrows[a0:t1] = r["nrows"].cpu().numpy()
        out.update(nrows=nrows, dates_idx=r["dates_idx"] + np.int32(a0), years=r["years"],
                   year0=r["year0"], features=names)
        return out

    def _gbt_rows(self, t1):
        """(rows_t, rows_a) int32: the z-score rows of the dates [0, t1), date-major."""
        import torch
        bits = self.zrows                                                # [nch][lda]
        sh = torch.arange(64, device=bits.device, dtype=torch.int64)
        m = ((bits[:, None, :] >> sh[None, :, None]) & 1).reshape(-1, bits.shape[1])[:t1]
        idx = torch.nonzero(m)
        return idx[:, 0].to(torch.int32).contiguous(), idx[:, 1].to(torch.int32).contiguous()

    def gbt_fit(self, params=None, *, rows: str = "train"):
        """Boosted regression trees (``afm.gbt``) on the last ``step()``'s panel (one GPU): the
        reference's XGBoost fits on the z-scored design.  The z statistics are the train window's
        and z is computed where it is read; the rows are the z-score rows (``zrows``); the label
        is the target plane.

        ``rows="train"`` (KKT:499-513): the dates [0, tr1) train (weight 1) and the valid dates
        not in train are scored every round (weight 0) -- ``model.evals`` and ``best_round``.
        ``rows="train+valid"`` (KKT:644-652): the dates [0, v1) train, train_end's rows twice
        where the reference's inclusive slices count that date twice (``Split.dup``).

        Runs on the caller's stream.  Returns a ``GBTModel``; the device results of the fit stay
        in ``self.gbt`` (``F``, the row lists ``rows_t`` / ``rows_a``, ``w``, ``bins``, ...)."""
        import torch
        from .gbt import GBTModel, _check_params, fit_device
        if self.W > 1:
            raise NotImplementedError("gbt_fit() runs on one GPU (world = 1)")
        params = _check_params(params)
        if rows not in ("train", "train+valid"):
            raise ValueError(f"rows={rows!r}: expected 'train' or 'train+valid'")
        if not self._stepped:
            raise ValueError("gbt_fit(): run step() first (the panel is empty)")
        sp, T, lda, dev = self.sp, self.T, self.lda, self.out.device
        with self.ctx.on(torch.cuda.current_stream(dev)):                    # the caller's stream
            rt, ra = self._gbt_rows(sp.v1)
            n = int(rt.numel())
            if n == 0:
                raise ValueError("gbt_fit(): the split has no z-score rows")
            if rows == "train":
                w = (rt < sp.tr1).to(torch.int32)
            else:
                w = torch.ones(n, dtype=torch.int32, device=dev)
                if sp.dup:
                    w += (rt == sp.tr1 - 1).to(torch.int32)
            y = torch.empty(n, dtype=torch.float64, device=dev)
            tcol = torch.tensor([TARGET], dtype=torch.int32, device=dev)
            self.ctx.call("afm_gbt_values_f64", self.out, T * lda, T, lda, tcol, 0, None, rt, ra,
                          n, y)
            ok = torch.isfinite(y)
            if not bool(ok.all()):                   # a row without a label neither trains nor scores
                rt, ra, w, y = rt[ok].contiguous(), ra[ok].contiguous(), w[ok].contiguous(), y[ok]
                n = int(rt.numel())
            res = fit_device(self.out, self.feat, y, w, params, T=T, lda=lda, n=n, zs=self.zs,
                             rows_t=rt, rows_a=ra, col_stride=T * lda)
            res.update(rows_t=rt, rows_a=ra, w=w, y=y)
            self.gbt = res
            return GBTModel.from_device(res, params, self.features)

    def gbt_predict(self, model, n_trees=None, frame: bool = False):
        """The trees of ``model`` (the first ``n_trees``; default all) walked over the test dates'
        z-score rows of the resident panel: a device plane [T][lda] shaped like ``pipe.pred`` --
        the prediction on those rows, NaN everywhere else.  ``frame=True``: the (date, id)-indexed
        one-column frame ('pred') that ``afm.AlphaSignalAnalyzer`` and ``afm.PortfolioManager``
        take (KKT:575, 991)."""
        import torch
        from .gbt import GBTModel, _n_trees
        if self.W > 1:
            raise NotImplementedError("gbt_predict() runs on one GPU (world = 1)")
        if not isinstance(model, GBTModel):
            raise TypeError(f"model: expected a GBTModel, got {type(model).__name__}")
        if list(model.features) != list(self.features):
            raise ValueError("gbt_predict(): the model was fit on other features than this "
                             "pipeline's")
        if not self._stepped:
            raise ValueError("gbt_predict(): run step() first (the panel is empty)")
        sp, T, lda, dev = self.sp, self.T, self.lda, self.out.device
        pred = torch.full((T, lda), float("nan"), dtype=torch.float64, device=dev)
        feat, thr, val = model.device_trees(dev)
        with self.ctx.on(torch.cuda.current_stream(dev)):
            self.ctx.call("afm_gbt_predict_f64", self.out, T * lda, lda, sp.s0, T - sp.s0,
                          self.feat, self.p, self.zs, feat, thr, val, model.params.max_depth,
                          _n_trees(model, n_trees), model.params.base_score, self.zrows, pred)
        if not frame:
            return pred
        import pandas as pd
        h = pred[:, :self.A].cpu().numpy()
        t, a = np.nonzero(~np.isnan(h))
        idx = pd.MultiIndex.from_arrays([np.asarray(self.full.dates)[t],
                                         np.asarray(self.full.ids)[a]], names=["date", "id"])
        return pd.DataFrame({"pred": h[t, a]}, index=idx)

    def gbt_contribs(self, model, n_trees=None, *, split: str = "test", rows: bool = False):
        """What the predictions of ``model`` (its first ``n_trees`` trees; default all) are made
        of on the z-score rows of a split of the resident panel (one GPU): the exact
        path-dependent TreeSHAP contributions (``afm.gbt``, include/afm_gbt_shap.h), aggregated
        per date on the device.  ``split``: 'train' (the dates [0, tr1)), 'valid' (the valid
        dates not in train, [tr1, v1)) or 'test' ([s0, T)).

        Returns a dict: ``by_date`` (a frame, dates x features + 'bias': the mean |phi| over the
        date's rows; NaN on a date without rows), ``mean_by_date`` (the same shape: the mean phi),
        ``importance`` (a Series over the features: the mean |phi| over all rows of the split,
        sorted descending), ``n`` (a Series: the rows per date) and, with ``rows=True``,
        ``contrib``: the device planes [nt][p + 1][lda] (date, column with the bias last, asset;
        NaN off the rows).  ``contrib`` takes nt * (p + 1) * lda * 8 bytes -- 4.8 GB for the 605
        test dates of the 10,000 x 5,040 configuration with its 97 columns, about 8 GB per 1,000
        dates -- which is why it is off by default."""
        import pandas as pd
        import torch
        from .gbt import GBTModel, _n_trees, check_cover, shap_device
        if self.W > 1:
            raise NotImplementedError("gbt_contribs() runs on one GPU (world = 1)")
        if not isinstance(model, GBTModel):
            raise TypeError(f"model: expected a GBTModel, got {type(model).__name__}")
        if split not in ("train", "valid", "test"):
            raise ValueError(f"split={split!r}: expected 'train', 'valid' or 'test'")
        if list(model.features) != list(self.features):
            raise ValueError("gbt_contribs(): the model was fit on other features than this "
                             "pipeline's")
        if not self._stepped:
            raise ValueError("gbt_contribs(): run step() first (the panel is empty)")
        R = _n_trees(model, n_trees)
        check_cover(model, R)
        sp, T, lda, dev = self.sp, self.T, self.lda, self.out.device
        t0, t1 = {"train": (0, sp.tr1), "valid": (sp.tr1, sp.v1), "test": (sp.s0, T)}[split]
        if t1 <= t0:
            raise ValueError(f"gbt_contribs(): the {split} split has no dates")
        with self.ctx.on(torch.cuda.current_stream(dev)):
            out = shap_device(self.ctx, model, R, self.out, T * lda, lda, t0, t1 - t0, self.feat,
                              self.p, self.zs, self.zrows, contrib=rows, agg=True)
            agg, cnt = out["agg"].cpu().numpy(), out["cnt"].cpu().numpy()
        names = list(self.features) + ["bias"]
        dates = pd.Index(np.asarray(self.full.dates)[t0:t1], name="date")
        with np.errstate(all="ignore"):
            per = agg / cnt[:, None, None].astype(np.float64)
            imp = agg[:, :self.p, 1].sum(axis=0) / float(cnt.sum())
        res = {"by_date": pd.DataFrame(per[:, :, 1], index=dates, columns=names),
               "mean_by_date": pd.DataFrame(per[:, :, 0], index=dates, columns=names),
               "importance": pd.Series(imp, index=list(self.features)).sort_values(
                   ascending=False, kind="stable"),
               "n": pd.Series(cnt, index=dates)}
        if rows:
            res["contrib"] = out["contrib"]
        return res

    def selected_features(self, model, k: int = 10, *, by: str = "weight",
                          split: str = "valid") -> list:
        """The reference's ``selected_features`` (KKT:545-554, 637): the ``k`` most-split columns
        of ``model`` united with the columns the step's Lasso kept, in ``FEATURES`` order.
        ``by="shap"``: the ``k`` columns of largest mean |phi| on ``split`` (``gbt_contribs``'s
        ``importance``; columns with none are left out) in place of the most-split ones."""
        if self.W > 1:
            raise NotImplementedError("selected_features() runs on one GPU (world = 1)")
        if by not in ("weight", "shap"):
            raise ValueError(f"by={by!r}: expected 'weight' or 'shap'")
        if not self._stepped:
            raise ValueError("selected_features(): run step() first (no Lasso fit)")
        if by == "shap":
            imp = self.gbt_contribs(model, split=split)["importance"]
            top = [f for f in imp.index[:k] if imp[f] > 0]
        else:
            top = model.top_features(k)
        beta = self.lasso_beta.cpu().numpy()
        keep = set(top) | {f for f, b in zip(self.features, beta[1:]) if b != 0}
        return [f for f in self.features if f in keep]

    def _net_fit_rows(self, rt, ra, what):
        """The train / eval rows of the network fits (``mlp_fit``, ``lstm_fit``) from the date-major
        rows (rt, ra) of the dates [0, v1): the rows of the dates [0, tr1), then those of [tr1 -
        dup, v1), without the rows that have no finite label.  -> rt, ra, y [n], n_train."""
        import torch
        sp, T, lda, dev = self.sp, self.T, self.lda, self.out.device
        ev = rt >= sp.tr1 - int(bool(sp.dup))
        tr = rt < sp.tr1
        rt = torch.cat([rt[tr], rt[ev]]).contiguous()
        ra = torch.cat([ra[tr], ra[ev]]).contiguous()
        n_train, n = int(tr.sum()), int(rt.numel())
        y = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        tcol = torch.tensor([TARGET], dtype=torch.int32, device=dev)
        if n:
            self.ctx.call("afm_gbt_values_f64", self.out, T * lda, T, lda, tcol, 0, None, rt,
                          ra, n, y)
        ok = torch.isfinite(y[:n])
        if not bool(ok.all()):                   # a row without a label neither trains nor scores
            n_train = int(ok[:n_train].sum())
            rt, ra, y = rt[ok].contiguous(), ra[ok].contiguous(), y[:n][ok]
        if n_train == 0:
            raise ValueError(f"{what}(): the split has no z-score rows to train on")
        return rt, ra, y[:int(rt.numel())], n_train

    def _net_fit(self, rt, ra, what, planes, fit_device, params):
        """A network fit on the rows of ``_net_fit_rows``: ``planes(rt, ra, n_pad)`` builds the
        design, the label is zero padded.  -> the device results of ``fit_device`` with the rows,
        ``X``, ``y``, ``n_train`` and ``n_eval`` added."""
        import torch
        rt, ra, y, n_train = self._net_fit_rows(rt, ra, what)
        n = int(rt.numel())
        n_pad = (n + 63) // 64 * 64
        X = planes(rt, ra, n_pad)
        yp = torch.zeros(n_pad, dtype=torch.float64, device=self.out.device)
        yp[:n] = y
        res = fit_device(X, yp, n_train, n - n_train, params)
        res.update(rows_t=rt, rows_a=ra, X=X, y=yp, n_train=n_train, n_eval=n - n_train)
        return res

    def _net_predict(self, rt, ra, planes, forward, member, frame):
        """The prediction plane [T][lda] of a network ensemble on those of the date-major rows (rt,
        ra) that lie in the test dates -- ``forward(planes(rt, ra, n_pad), n)`` -> [M][n_pad], the
        member or the member mean scattered, NaN everywhere else -- or, with ``frame``, the (date,
        id)-indexed one-column frame ('pred')."""
        import torch
        T, lda, dev = self.T, self.lda, self.out.device
        pred = torch.full((T, lda), float("nan"), dtype=torch.float64, device=dev)
        te = rt >= self.sp.s0
        rt, ra = rt[te].contiguous(), ra[te].contiguous()
        n = int(rt.numel())
        if n:
            out = forward(planes(rt, ra, (n + 63) // 64 * 64), n)
            val = out[member, :n] if member is not None else out[:, :n].mean(dim=0)
            pred[rt.long(), ra.long()] = val
        if not frame:
            return pred
        import pandas as pd
        h = pred[:, :self.A].cpu().numpy()
        t, a = np.nonzero(~np.isnan(h))
        idx = pd.MultiIndex.from_arrays([np.asarray(self.full.dates)[t],
                                         np.asarray(self.full.ids)[a]], names=["date", "id"])
        return pd.DataFrame({"pred": h[t, a]}, index=idx)

    def _mlp_columns(self, features):
        """The indices into ``self.features`` of the named columns (default: all)."""
        if features is None:
            return list(range(len(self.features)))
        if isinstance(features, (str, bytes)):
            raise TypeError("features: expected a list of column names")
        features = [str(f) for f in features]
        unknown = [f for f in features if f not in self.features]
        if unknown:
            raise ValueError(f"unknown features {unknown}: not among this pipeline's")
        if not features or len(set(features)) != len(features):
            raise ValueError("features: expected distinct column names, at least one")
        return [self.features.index(f) for f in features]

    def _mlp_planes(self, idx, rt, ra, n_pad):
        """The z-scored design of the rows (rt, ra) as planes [len(idx)][n_pad], zero padded: one
        afm_gbt_values_f64 per column, at the column's own index in ``self.feat`` / ``self.zs``."""
        import torch
        T, lda, n = self.T, self.lda, int(rt.numel())
        X = torch.zeros((len(idx), n_pad), dtype=torch.float64, device=self.out.device)
        for j, k in enumerate(idx):
            self.ctx.call("afm_gbt_values_f64", self.out, T * lda, T, lda, self.feat, k, self.zs,
                          rt, ra, n, X[j])
        return X

    def mlp_fit(self, params=None, *, features=None):
        """An ensemble of small dense networks (``afm.mlp``) on the last ``step()``'s panel (one
        GPU): the reference's Dense(128) -> Dense(32) -> Dense(1) fit (KKT:668-684) on the z-scored
        design.  The rows of the dates [0, tr1) train, date-major and unshuffled; the rows of the
        dates [tr1 - dup, v1) are scored at the end of every epoch -- the reference's ``df_valid``
        starts on train_end itself (``Split.dup``); rows without a finite label are dropped.
        ``features``: the columns to fit on (default: all of ``self.features``); the reference's
        call is ``pipe.mlp_fit(features=pipe.selected_features(gbt_model))``.

        Runs on the caller's stream.  Returns a ``MLPModel``; the device results of the fit stay
        in ``self.mlp`` (``theta``, ``evals``, ``snaps``, ``X``, ``y``, the row lists ``rows_t`` /
        ``rows_a``, ``n_train``, ``n_eval``)."""
        import torch
        from .mlp import MLPModel, _check_params, _check_shape, fit_device
        if self.W > 1:
            raise NotImplementedError("mlp_fit() runs on one GPU (world = 1)")
        params = _check_params(params)
        if not self._stepped:
            raise ValueError("mlp_fit(): run step() first (the panel is empty)")
        idx = self._mlp_columns(features)
        _check_shape(len(idx), params.hidden)
        dev = self.out.device
        with self.ctx.on(torch.cuda.current_stream(dev)):                    # the caller's stream
            rt, ra = self._gbt_rows(self.sp.v1)
            res = self._net_fit(rt, ra, "mlp_fit",
                                lambda t, a, n_pad: self._mlp_planes(idx, t, a, n_pad), fit_device,
                                params)
            self.mlp = res
            return MLPModel.from_device(res, params, [self.features[k] for k in idx])

    def mlp_predict(self, model, frame: bool = False, member=None):
        """The networks of ``model`` over the test dates' z-score rows of the resident panel: a
        device plane [T][lda] shaped like ``pipe.pred`` -- the mean over the members (default) or
        the prediction of ``member`` on those rows, NaN everywhere else.  ``frame=True``: the
        (date, id)-indexed one-column frame ('pred') that ``afm.AlphaSignalAnalyzer`` and
        ``afm.PortfolioManager`` take (KKT:686-706)."""
        import torch
        from .mlp import MLPModel, _member, forward_device
        if self.W > 1:
            raise NotImplementedError("mlp_predict() runs on one GPU (world = 1)")
        if not isinstance(model, MLPModel):
            raise TypeError(f"model: expected a MLPModel, got {type(model).__name__}")
        if not self._stepped:
            raise ValueError("mlp_predict(): run step() first (the panel is empty)")
        idx = self._mlp_columns(model.features)
        member = _member(model, member)
        dev = self.out.device
        with self.ctx.on(torch.cuda.current_stream(dev)):
            rt, ra = self._gbt_rows(self.T)
            return self._net_predict(
                rt, ra, lambda t, a, n_pad: self._mlp_planes(idx, t, a, n_pad),
                lambda X, n: forward_device(X, model.device_theta(dev), model.params.hidden, 0, n),
                member, frame)

    # ---- stacked LSTM ensembles (afm.lstm, include/afm_lstm.h; one GPU) ----------------------------
    def _lstm_rows(self, t1, lookback):
        """(rows_t, rows_a) int32, date-major: the z-score rows of the dates [0, t1) -- with
        ``lookback=L`` only those whose asset has a z-score row on all of the L dates up to
        theirs."""
        import torch
        rt, ra = self._gbt_rows(t1)
        if lookback is None:
            return rt, ra
        m = torch.zeros((t1, self.zrows.shape[1]), dtype=torch.bool, device=rt.device)
        m[rt.long(), ra.long()] = True
        win = m.clone()
        for k in range(1, lookback):
            win[k:] &= m[:t1 - k]
        win[:lookback - 1] = False
        idx = torch.nonzero(win)
        return idx[:, 0].to(torch.int32).contiguous(), idx[:, 1].to(torch.int32).contiguous()

    def _lstm_planes(self, idx, rt, ra, n_pad, lookback):
        """The z-scored sequences of the rows (rt, ra) as planes [T][d][n_pad], zero padded.
        ``lookback=None``: T = len(idx), d = 1 -- ``_mlp_planes``' output; ``lookback=L``: plane
        (t, j) is column idx[j] at the date L - 1 - t before the row's, gathered with
        afm_gbt_values_f64 on the shifted row list."""
        import torch
        if lookback is None:
            return self._mlp_planes(idx, rt, ra, n_pad).view(len(idx), 1, n_pad)
        T, lda, n = self.T, self.lda, int(rt.numel())
        X = torch.zeros((lookback, len(idx), n_pad), dtype=torch.float64, device=self.out.device)
        for t in range(lookback):
            st = (rt - (lookback - 1 - t)).contiguous()
            for j, k in enumerate(idx):
                self.ctx.call("afm_gbt_values_f64", self.out, T * lda, T, lda, self.feat, k,
                              self.zs, st, ra, n, X[t, j])
        return X

    def _lstm_layout(self, n_features, lookback):
        from .lstm import MAX_STEPS, _check_shape
        if lookback is not None:
            try:
                lookback = operator.index(lookback)
            except TypeError:
                raise ValueError(f"lookback={lookback!r}: expected an integer or None") from None
            if not 1 <= lookback <= MAX_STEPS:
                raise ValueError(f"lookback={lookback}: expected 1..{MAX_STEPS}")
            _check_shape(lookback, n_features)
        else:
            _check_shape(n_features, 1)
        return lookback

    def lstm_fit(self, params=None, *, features=None, lookback=None):
        """An ensemble of stacked LSTMs (``afm.lstm``) on the last ``step()``'s panel (one GPU):
        the reference's LSTM -> LSTM -> Dense(1) fits (KKT:709-789) on the z-scored design, with
        the train / eval rows of ``mlp_fit``.  ``lookback=None`` is the reference's layout: every
        feature is one step (``T = len(features), d = 1``).  ``lookback=L``: a row is the window of
        the last L dates of its security (``T = L, d = len(features)``); it is kept only if the
        asset has a z-score row on all L dates.  The windows of eval rows may reach back across the
        split boundary: features of earlier dates are not a look-ahead.

        Runs on the caller's stream.  Returns a ``LSTMModel`` (it remembers ``lookback``); the
        device results of the fit stay in ``self.lstm`` (``theta``, ``evals``, ``snaps``, ``X``,
        ``y``, the row lists ``rows_t`` / ``rows_a``, ``n_train``, ``n_eval``)."""
        import torch
        from .lstm import LSTMModel, _check_params, fit_device
        if self.W > 1:
            raise NotImplementedError("lstm_fit() runs on one GPU (world = 1)")
        params = _check_params(params)
        if not self._stepped:
            raise ValueError("lstm_fit(): run step() first (the panel is empty)")
        idx = self._mlp_columns(features)
        lookback = self._lstm_layout(len(idx), lookback)
        dev = self.out.device
        with self.ctx.on(torch.cuda.current_stream(dev)):                    # the caller's stream
            rt, ra = self._lstm_rows(self.sp.v1, lookback)
            res = self._net_fit(
                rt, ra, "lstm_fit",
                lambda t, a, n_pad: self._lstm_planes(idx, t, a, n_pad, lookback), fit_device,
                params)
            self.lstm = res
            return LSTMModel.from_device(res, params, [self.features[k] for k in idx], lookback)

    def lstm_predict(self, model, frame: bool = False, member=None):
        """The networks of ``model`` over the test dates' z-score rows of the resident panel (with
        ``model.lookback``: those with a full window, rebuilt as ``lstm_fit`` built them): a device
        plane [T][lda] shaped like ``pipe.pred`` -- the mean over the members (default) or the
        prediction of ``member`` on those rows, NaN everywhere else.  ``frame=True``: the (date,
        id)-indexed one-column frame ('pred') that ``afm.AlphaSignalAnalyzer`` and
        ``afm.PortfolioManager`` take."""
        import torch
        from .lstm import LSTMModel, forward_device
        from .mlp import _member
        if self.W > 1:
            raise NotImplementedError("lstm_predict() runs on one GPU (world = 1)")
        if not isinstance(model, LSTMModel):
            raise TypeError(f"model: expected a LSTMModel, got {type(model).__name__}")
        if not self._stepped:
            raise ValueError("lstm_predict(): run step() first (the panel is empty)")
        idx = self._mlp_columns(model.features)
        member = _member(model, member)
        dev = self.out.device
        with self.ctx.on(torch.cuda.current_stream(dev)):
            rt, ra = self._lstm_rows(self.T, model.lookback)
            return self._net_predict(
                rt, ra, lambda t, a, n_pad: self._lstm_planes(idx, t, a, n_pad, model.lookback),
                lambda X, n: forward_device(X, model.device_theta(dev), model.params.hidden, 0, n),
                member, frame)

    # ---- the factor risk model (afm.risk, include/afm_risk.h; one GPU) ----------------------------
    def risk_fit(self, params=None, features=None, rows: str = "z"):
        """The multi-factor risk model (``afm.risk``) on the last ``step()``'s panel (one GPU): the
        per-date regressions of the target plane on the raw planes ``features`` (default:
        ``cfg.fm_features``, the Fama-MacBeth design) over the z-score rows (``rows="z"``) or the
        all_df rows (``rows="alldf"``) of ALL dates -- its own afm_xs_gram_f64 + afm_ols_solve_f64,
        the step's FM buffers are not touched -- then the EWMA factor covariance, the residuals and
        the EWMA specific variance.  Runs on the caller's stream.  Returns a ``RiskModel``; the
        device results (the residual plane among them) stay in ``self.risk``."""
        import torch
        from .risk import RiskModel, _check_factors, _check_params, fit_device
        if self.W > 1:
            raise NotImplementedError("risk_fit() runs on one GPU (world = 1)")
        params = _check_params(params)
        if rows not in ("z", "alldf"):
            raise ValueError(f"rows={rows!r}: expected 'z' or 'alldf'")
        names = list(self.cfg.fm_features) if features is None else [str(f) for f in features]
        unknown = [f for f in names if f not in COL]
        if unknown or len(set(names)) != len(names):
            raise ValueError(f"features: unknown or repeated columns {unknown}")
        _check_factors(len(names))
        if not self._stepped:
            raise ValueError("risk_fit(): run step() first (the panel is empty)")
        T, lda, dev = self.T, self.lda, self.out.device
        with self.ctx.on(torch.cuda.current_stream(dev)):                    # the caller's stream
            res = fit_device(self.out, [COL[f] for f in names], TARGET,
                             self.zrows if rows == "z" else self.alldf, params, T=T, A=self.A,
                             lda=lda, col_stride=T * lda, tol=self.cfg.tol)
        self.risk = res
        return RiskModel(params, names, self.full.dates, self.full.ids, res)

    def _risk_model(self, model, what):
        from .risk import RiskModel
        if not isinstance(model, RiskModel):
            raise TypeError(f"model: expected a RiskModel, got {type(model).__name__}")
        if tuple(model["fcov"].shape[:1]) != (self.T,) or tuple(model["spec"].shape) != \
                (self.T, self.lda):
            raise ValueError(f"{what}: the model was fit on another panel than this pipeline's")
        if not self._stepped:
            raise ValueError(f"{what}: run step() first (the panel is empty)")

    def book_risk(self, model, reb=None):
        """The books of a rebalance (default: the last step's, ``self.reb``) priced by ``model`` at
        the rebalance dates (one GPU).  Returns a frame per date: the predicted volatility (the
        square root of the variance per period) ``long_vol`` / ``long_factor_vol`` /
        ``long_specific_vol`` and the same for ``short_`` and ``net_`` (the net book is
        (long - short) / 2), ``long_filled`` ... (members priced at the date's mean specific
        variance), ``status`` (4: the model has no forecast for the date), and ``contrib``: a frame
        with the columns (book, factor), the factors' contributions to the factor variance.  The
        device results stay in ``self.risk_books``."""
        import pandas as pd
        import torch
        from .risk import book_risk_device
        if self.W > 1:
            raise NotImplementedError("book_risk() runs on one GPU (world = 1)")
        self._risk_model(model, "book_risk()")
        reb = self.reb if reb is None else reb
        dev = self.out.device
        with self.ctx.on(torch.cuda.current_stream(dev)):
            out = book_risk_device(model.planes, self.out, reb, self.rdates, T=self.T,
                                   lda=self.lda, kc=max(int(self.cfg.top_n), 1),
                                   col_stride=self.T * self.lda)
        self.risk_books = out
        risk, contrib = out["risk"].cpu().numpy(), out["contrib"].cpu().numpy()
        dates = pd.Index(np.asarray(self.full.dates)[self.rdates.cpu().numpy()], name="date")
        cols = {}
        with np.errstate(all="ignore"):
            for s, book in enumerate(("long", "short", "net")):
                for j, part in enumerate(("vol", "factor_vol", "specific_vol")):
                    cols[f"{book}_{part}"] = np.sqrt(risk[:, s, j])
                cols[f"{book}_filled"] = risk[:, s, 3]
        cols["status"] = out["status"].cpu().numpy()
        frame = pd.DataFrame(cols, index=dates)
        ci = pd.MultiIndex.from_product([("long", "short", "net"), model.factors],
                                        names=["book", "factor"])
        frame.attrs["contrib"] = pd.DataFrame(contrib.reshape(len(dates), -1), index=dates,
                                              columns=ci)
        return frame

    def risk_rebalance(self, model, risk_tolerance: float = 0.0, mu=None, v0=None, rate=None):
        """The rebalance with the model's covariance in place of the sample covariance (one GPU):
        the existing rebalance for the selection (and the sample-covariance weights), the books'
        covariance B F B' + D, every book's weights solved again from it, then the PnL scan.
        ``risk_tolerance`` > 0 adds the return term with ``mu`` a [T][lda] device plane (default:
        the prediction plane).  A date the model has no forecast for keeps the sample-covariance
        weights (status bit 4).  Returns a dict of device tensors: the rebalance arrays (k, books,
        weights, sums, upos, usize, status), the scan's (value, turnover, long_ret, short_ret) and
        ``cov`` / ``cov_status``; ``self.reb`` and ``self.pnl`` are not touched."""
        import torch
        from .portfolio import pnl_scan, rebalance
        from .risk import book_risk_device, rebalance_cov_device
        if self.W > 1:
            raise NotImplementedError("risk_rebalance() runs on one GPU (world = 1)")
        self._risk_model(model, "risk_rebalance()")
        c, sp, full, dev = self.cfg, self.sp, self.full, self.out.device
        gamma = float(risk_tolerance)
        if not gamma >= 0 or not np.isfinite(gamma):
            raise ValueError(f"risk_tolerance={risk_tolerance!r}: expected a finite number >= 0")
        mu = (self.pred if mu is None else mu) if gamma > 0 else None
        kc = max(int(c.top_n), 1)
        with self.ctx.on(torch.cuda.current_stream(dev)):
            reb = rebalance(self.pred, full.tbits, self.target, self.zrows_full, full.close,
                            self.tmr, self.rdates, A=full.A, top_n=c.top_n, window=c.window,
                            h_range=(0, sp.tr1), lo=c.lo, hi=c.hi)
            cv = book_risk_device(model.planes, self.out, reb, self.rdates, T=self.T, lda=self.lda,
                                  kc=kc, col_stride=self.T * self.lda)
            rebalance_cov_device(reb, cv["cov"], self.rdates, full.close, self.tmr, kc=kc,
                                 cov_status=cv["status"], mu=mu, risk_tolerance=gamma, lo=c.lo,
                                 hi=c.hi)
            res = pnl_scan(reb, c.v0 if v0 is None else v0, c.rate if rate is None else rate)
        res.update(reb, cov=cv["cov"], cov_status=cv["status"])
        return res

    def summary(self) -> dict:
        """Host copies of the headline results (after a synchronize)."""
        v = self.pnl["value"].cpu().numpy()
        r = v[1:] / v[:-1] - 1
        out = {"final_value": float(v[-1]), "sharpe": float(r.mean() / r.std(ddof=1)),
               "lasso_beta": self.lasso_beta.cpu().numpy(),
               "lasso_n_iter": int(self.lasso_info[2].item()),
               "lasso_nnz": int((self.lasso_beta[1:] != 0).sum().item()),
               "fm_mean": self.fm_mean.cpu().numpy(), "fm_t": self.fm_t.cpu().numpy(),
               "fm_rank": self.fm_rank.cpu().numpy(), "k": self.reb["k"].cpu().numpy(),
               "status": self.reb["status"].cpu().numpy()}
        if self.cfg.analyzer:
            ic = self.an["ic"].cpu().numpy()
            out["ic_mean"] = np.nanmean(ic, axis=0)
        return out
