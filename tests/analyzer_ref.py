"""References of the signal-evaluation and ingest kernels (csrc/analyzer.hip) for the direct
kernel tests: the reference's own pandas / numpy statement on the same rows ("KKT Yuliang
Jiang.py", cited as KKT:line), per date where the statement is per date.  Where a few lines of
numpy stand in for a pandas statement, tests/test_analyzer_ref.py pins them to it on the CPU.
Also the input builders the CPU and the GPU tests share.  Nothing here touches the GPU."""
import warnings

import numpy as np
import pandas as pd

RETURNS = ("return_1", "return_2", "return_5")        # KKT:290
KS = (1, 2, 5)
COLS = ["f"] + list(RETURNS)
NP_BUF = 8192                                         # numpy's ufunc reduction buffer (elements)


# ---- grids --------------------------------------------------------------------------------------
def pack_bits(present: np.ndarray) -> np.ndarray:
    """[T][lda] bool -> [ceil(T/64)][lda] int64 words; bit s of word [c][a] = day 64c + s."""
    T, lda = present.shape
    nch = (T + 63) // 64
    p = np.zeros((nch * 64, lda), dtype=np.uint64)
    p[:T] = present
    sh = np.arange(64, dtype=np.uint64).reshape(1, 64, 1)
    return (p.reshape(nch, 64, lda) << sh).sum(axis=1, dtype=np.uint64).view(np.int64)


def mixed_scale(rng, shape):
    """Values of mixed sign over 1e-4 .. 1e4: a sum in another order rounds differently."""
    return rng.normal(size=shape) * 10.0 ** rng.uniform(-4, 4, shape)


# ---- sums ---------------------------------------------------------------------------------------
def np_mean(v: np.ndarray) -> float:
    """Series.mean() of a NaN-free column: numpy's own reduction of a contiguous copy / count."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    return np.add.reduce(v) / len(v) if len(v) else np.nan


def np_nanmean(v: np.ndarray) -> float:
    """Series.mean() (nanops.nanmean): the sum with NaN -> 0 over the non-NaN count."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    bad = np.isnan(v)
    cnt = len(v) - int(bad.sum())
    return np.add.reduce(np.where(bad, 0.0, v)) / cnt if cnt else np.nan


def one_tree_sum(v: np.ndarray) -> float:
    """What a sum would be as ONE numpy pairwise tree over the whole vector (not numpy's result
    past 8192 elements): the alternative the multi-buffer cases must tell apart."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    n = len(v)
    if n <= NP_BUF:                    # within one buffer numpy's reduction is this tree
        return float(np.add.reduce(v)) if n else 0.0
    n2 = n // 2
    n2 -= n2 % 8
    return one_tree_sum(v[:n2]) + one_tree_sum(v[n2:])


# ---- A1: forward returns (KKT:311-312) -------------------------------------------------------------
def fwd_returns_ref(close: np.ndarray, present: np.ndarray) -> np.ndarray:
    """[3][T][lda]: per asset over its present days, close[i+k] / close[i] - 1, NaN unless <= 1;
    absent cells NaN."""
    T, lda = close.shape
    fr = np.full((3, T, lda), np.nan)
    for a in range(lda):
        days = np.flatnonzero(present[:, a])
        c = close[days, a]
        for q, k in enumerate(KS):
            if len(c) > k:
                with np.errstate(all="ignore"):
                    v = c[k:] / c[:-k] - 1
                fr[q, days[:-k], a] = np.where(v <= 1, v, np.nan)
    return fr


def fwd_returns_pandas(close_col: np.ndarray, k: int) -> np.ndarray:
    """One asset's price rows in date order -> KKT:311-312's column (NaN where the row is cut)."""
    s = pd.Series(close_col).pct_change(k).shift(-k).to_frame("r")
    s = s[s["r"] <= 1]
    return s["r"].reindex(range(len(close_col))).to_numpy()


def fwd_inputs(seed=5, T=197, lda=128):
    """close, present of the forward-return cases: asset 0 every day; 1 only days 63, 64, 127,
    128; 2 a gap of more than 128 days (an empty presence word between two present days); 3 its
    last rows closer than 5 to the end; 4 never; 5 prices 1, 2, nextafter(2) on consecutive rows
    (a return of exactly 1.0 kept, the smallest one above 1 cut); the rest present with p = 0.5."""
    rng = np.random.default_rng(seed)
    present = rng.random((T, lda)) < 0.5
    close = 30 * np.exp(rng.normal(0, 0.3, (T, lda)))
    present[:, 0] = True
    present[:, 1] = False
    present[[63, 64, 127, 128], 1] = True
    present[:, 2] = False
    present[[3, 40, 62, 193, 195, 196], 2] = True         # words 0 and 3 only
    present[:, 3] = False
    present[[10, 11, 12, 190, 191, 194, 196], 3] = True
    present[:, 4] = False
    present[:, 5] = True
    # day 60 -> 61: 2 / 1 - 1 == 1.0 (kept); day 60 -> 62: the quotient is the next double above
    # 2, so the return is 1 + 2**-51, the smallest c'/c - 1 above 1 (cut)
    close[60:66, 5] = [1.0, 2.0, np.nextafter(2.0, 3.0), 4.0, 4.0, 4.0]
    return close, present


# ---- A1: merge / dropna cascade + per-date demean (KKT:313-318) -----------------------------------
def prepare_ref(sig: np.ndarray, fr: np.ndarray):
    """sig [T][A], fr [3][T][A] -> per date (asset index [n], rows [4][n]): keep_q = signal and
    returns 1..q non-NaN, mu_q = mean of return q over keep_q, the rows of keep_2 in ascending
    asset order with return q - mu_q."""
    out = []
    for t in range(sig.shape[0]):
        keep = ~np.isnan(sig[t])
        mu = []
        for q in range(3):
            keep = keep & ~np.isnan(fr[q, t])
            mu.append(np_mean(fr[q, t, keep]))
        idx = np.flatnonzero(keep)
        rows = np.stack([sig[t, idx]] + [fr[q, t, idx] - mu[q] for q in range(3)])
        out.append((idx.astype(np.int32), rows))
    return out


def prepare_pandas(sig_t: np.ndarray, fr_t: np.ndarray):
    """One date in the statements of KKT:313-318: per return type a left merge of the column,
    dropna, then x[rt] = x[rt] - x[rt].mean() -> (asset index, rows [4][n])."""
    df = pd.DataFrame({"id": np.arange(len(sig_t)), "f": sig_t})
    for q, rt in enumerate(RETURNS):
        ret = pd.DataFrame({"id": np.arange(len(sig_t)), rt: fr_t[q]})
        ret = ret.dropna()                                 # return_data holds no row there
        df = pd.merge(df, ret, on=["id"], how="left").dropna()
        df[rt] = df[rt] - df[rt].mean()
    return df["id"].to_numpy().astype(np.int32), df[COLS].to_numpy().T


PREP_COUNTS = (0, 1, 7, 8, 127, 128, 129, 8191, 8192, 8193, 16385, 1 << 30)   # last: every row


def prepare_inputs(A: int, lda: int, seed: int = 11):
    """sig [T][lda], fr [3][T][lda] (T = 12) whose date t keeps min(PREP_COUNTS[t], A) rows through
    all three steps; NaNs sit independently in the planes, so that the step masks differ (n0 > n1 >
    n2 where rows are left over) and each mean runs over its own step's rows.  The padding columns
    [A, lda) hold finite values the kernel must not read as rows."""
    rng = np.random.default_rng(seed)
    T = len(PREP_COUNTS)
    sig = mixed_scale(rng, (T, lda))
    fr = mixed_scale(rng, (3, T, lda))
    for t, c in enumerate(PREP_COUNTS):
        c = min(c, A)
        perm = rng.permutation(A)
        rest = perm[c:]
        e2 = len(rest) // 4 if c < A else 0               # lost at step 2 only
        e1 = len(rest) // 4 if c < A else 0               # lost at step 1
        fr[2, t, rest[:e2]] = np.nan
        fr[1, t, rest[e2:e2 + e1]] = np.nan
        fr[2, t, rest[e2:e2 + e1:2]] = np.nan
        tail = rest[e2 + e1:]                             # lost at step 0 or no signal row
        how = rng.integers(0, 3, len(tail))
        sig[t, tail[how != 1]] = np.nan
        fr[0, t, tail[how != 0]] = np.nan
        fr[1:, t, tail[::3]] = np.nan
    return sig, fr


# ---- A3/A4: ranks (KKT:328, 359) ---------------------------------------------------------------
def rank_ref(v: np.ndarray):
    """rank(method='first') ascending and descending of one date: 1..n, ties by row position."""
    n = len(v)
    ra, rd = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    ra[np.argsort(v, kind="stable")] = np.arange(1, n + 1)
    rd[np.argsort(-v, kind="stable")] = np.arange(1, n + 1)
    return ra, rd


def rank_pandas(v: np.ndarray):
    s = pd.Series(v)
    return (s.rank(method="first").to_numpy().astype(np.int32),
            s.rank(method="first", ascending=False).to_numpy().astype(np.int32))


def rank_values(rng, kind: str, shape):
    if kind == "normal":
        return rng.normal(size=shape)
    if kind == "ties":
        v = rng.integers(-3, 4, shape).astype(np.float64) * 0.25
        v[::2] = 1.5                                       # all-equal dates
        return v
    if kind == "zeros":
        v = rng.integers(-1, 2, shape).astype(np.float64)
        v[rng.random(shape) < 0.3] = -0.0                  # -0.0 ties with 0.0
        return v
    assert kind == "inf"
    v = np.round(rng.normal(size=shape), 2)
    u = rng.random(shape)
    v[u < 0.02] = np.inf
    v[u > 0.98] = -np.inf
    return v


# ---- A2-A4: per-date statistics (KKT:328-332, 344-345, 358-369) --------------------------------
def stats_pandas(dates_rows):
    """dates_rows: per evaluated date the rows [4][n] (factor, return_1, return_2, return_5) ->
    ic [nd][3], layer_mean [nd][3][10], layer_cnt [nd][10], port [nd][3], in pandas."""
    nd = len(dates_rows)
    ic = np.full((nd, 3), np.nan)
    lm = np.full((nd, 3, 10), np.nan)
    lc = np.zeros((nd, 10), dtype=np.int32)
    frames = []
    for i, r in enumerate(dates_rows):
        df = pd.DataFrame(dict(zip(COLS, r)))
        with np.errstate(all="ignore"):
            ic[i] = df.corr(method="pearson")["f"].to_numpy()[1:]            # KKT:344-345
        layer = (df["f"].rank(pct=True, method="first") * 10).astype(int) + 1   # KKT:328-330
        layer[layer > 10] = 10
        df["layer"] = layer
        with np.errstate(all="ignore"):
            for k, rt in enumerate(RETURNS):
                m = df.groupby("layer")[rt].mean()                           # KKT:331
                lm[i, k, m.index.to_numpy() - 1] = m.to_numpy()
        cnt = df.groupby("layer").size()
        lc[i, cnt.index.to_numpy() - 1] = cnt.to_numpy()
        df["date"] = i
        frames.append(df)
    port = np.zeros((nd, 3))
    if nd:
        pdf = pd.concat(frames, ignore_index=True)
        pdf["rank"] = pdf.groupby("date")["f"].rank(method="first", ascending=False)  # KKT:359
        pdf = pdf[pdf["rank"] <= 10].sort_values(by=["date", "rank"])
        pdf["rank"] = pdf["rank"].astype(str)
        with np.errstate(all="ignore"):
            w = pd.pivot(data=pdf, index="date", columns="rank", values="f")   # KKT:365-369
            w = w.div(w.sum(axis=1), axis=0)
            for k, rt in enumerate(RETURNS):
                ret = pd.pivot(data=pdf, index="date", columns="rank", values=rt)
                port[:, k] = ret.mul(w).sum(axis=1).reindex(range(nd)).to_numpy()
    return ic, lm, lc, port


STAT_COUNTS = (1, 2, 9, 10, 11, 511, 512, 513, 1025, 1537)


def stats_inputs(kind: str, lda: int = 1600, seed: int = 21):
    """rows [4][T][lda] with STAT_COUNTS rows per date.  Kinds: 'finite'; 'inf' (+-inf in the
    factor: first chunk of the 1025-row date, only the second chunk of the 1537-row date, the last
    row of the 513-row date, one of the two rows of the 2-row date); 'const' (a constant factor on
    the 11- and the 512-row dates); 'retinf' (inf in return columns)."""
    rng = np.random.default_rng(seed)
    T = len(STAT_COUNTS)
    rows = rng.normal(size=(4, T, lda))
    rows[0] = np.round(rows[0], 2)                          # ties in the factor
    rows[1:] *= 0.02
    t_of = {n: t for t, n in enumerate(STAT_COUNTS)}
    if kind == "inf":
        rows[0, t_of[1025], [5, 300]] = [np.inf, -np.inf]
        rows[0, t_of[1537], [512, 700, 1023]] = [np.inf, -np.inf, np.inf]
        rows[0, t_of[513], 512] = np.inf
        rows[0, t_of[2], 1] = -np.inf
        rows[0, t_of[10], 3] = np.inf
    elif kind == "const":
        rows[0, t_of[11]] = 0.75
        rows[0, t_of[512]] = -2.0
    elif kind == "retinf":
        rows[1, t_of[1537], 600] = np.inf
        rows[2, t_of[1537], [100, 1300]] = [np.inf, -np.inf]
        rows[3, t_of[513], 0] = -np.inf
        rows[1, t_of[11], np.argmax(rows[0, t_of[11], :11])] = np.inf   # a top-10 row
    else:
        assert kind == "finite"
    return rows, np.array(STAT_COUNTS, dtype=np.int32)


# ---- series (KKT:331-340, 351-354, 371) -------------------------------------------------------
def series_pandas(layer_mean, port, ic, year, nyears, year0):
    """-> cum_layer [nd][3][10], ls [nd][3][5], cum_port [nd][3], ir [nyears][3], in pandas."""
    nd = len(year)
    cum = np.empty((nd, 3, 10))
    ls = np.empty((nd, 3, 5))
    for k in range(3):
        c = pd.DataFrame(layer_mean[:, k, :], columns=range(1, 11)).cumsum()   # KKT:331-332
        cum[:, k, :] = c.to_numpy()
        for l in range(1, 6):                                                # KKT:337-339
            ls[:, k, l - 1] = (c[10 - l + 1] - c[l]).to_numpy()
    cum_port = pd.DataFrame(port).cumsum().to_numpy()                        # KKT:371
    ir = np.full((nyears, 3), np.nan)
    icdf = pd.DataFrame(ic, columns=list(RETURNS))
    icdf.index = pd.Index(year, name="year")
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        long = icdf.stack().reset_index()                                    # drops the NaN ICs
        long.columns = ["year", "Type", "IC"]
        if len(long):
            g = long.groupby(["year", "Type"]).apply(
                lambda x: x["IC"].mean() / x["IC"].std())                    # KKT:353
            for (y, tp), v in g.items():
                ir[int(y) - year0, RETURNS.index(tp)] = v
    return cum, ls, cum_port, ir


def series_inputs(years, seed=31, nan_frac=0.05):
    """Synthetic layer_mean / port / ic for the dates whose years are ``years``."""
    rng = np.random.default_rng(seed)
    nd = len(years)
    lm = mixed_scale(rng, (nd, 3, 10))
    lm[rng.random(lm.shape) < nan_frac] = np.nan
    port = mixed_scale(rng, (nd, 3))
    ic = rng.uniform(-1, 1, (nd, 3))
    ic[rng.random(ic.shape) < nan_frac] = np.nan
    return lm, port, ic, np.asarray(years, dtype=np.int32)


# ---- ingest (KKT:146-148, 158-161) ----------------------------------------------------------------
def ffill_pandas(planes: np.ndarray, present: np.ndarray) -> np.ndarray:
    """planes [K][T][lda]: per security its present rows in date order, .ffill() (KKT:146); absent
    cells as they were."""
    out = planes.copy()
    for a in range(planes.shape[2]):
        days = np.flatnonzero(present[:, a])
        if len(days):
            g = pd.DataFrame(planes[:, days, a].T).ffill()
            out[:, days, a] = g.to_numpy().T
    return out


def date_mean_fill_ref(planes: np.ndarray, present: np.ndarray) -> np.ndarray:
    """Per date and column over the date's present rows: NaN -> the column's mean (KKT:148)."""
    out = planes.copy()
    for k in range(planes.shape[0]):
        for t in range(planes.shape[1]):
            rows = np.flatnonzero(present[t])
            v = planes[k, t, rows]
            if len(rows) and np.isnan(v).any():
                out[k, t, rows] = np.where(np.isnan(v), np_nanmean(v), v)
    return out


def date_mean_fill_pandas(cols: np.ndarray) -> np.ndarray:
    """One date's rows [n][K] -> group.fillna(group.mean()) (KKT:148)."""
    g = pd.DataFrame(cols)
    return g.fillna(g.mean()).to_numpy()


def group_demean_ref(x: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    out = np.empty_like(x)
    for g in range(len(offsets) - 1):
        v = x[offsets[g]:offsets[g + 1]]
        out[offsets[g]:offsets[g + 1]] = v - np_nanmean(v)
    return out


def group_demean_pandas(v: np.ndarray) -> np.ndarray:
    s = pd.Series(v)
    return (s - s.mean()).to_numpy()                                         # KKT:159


# ---- the oracle's top_stocks pin (KKT:358-369) --------------------------------------------------
def top_stocks_pandas(date: np.ndarray, vals: np.ndarray) -> np.ndarray:
    """port [nd][3] of the rows (date, [factor, return_1, return_2, return_5])."""
    df = pd.DataFrame(vals, columns=COLS)
    df["date"] = date
    df["rank"] = df.groupby("date")["f"].rank(method="first", ascending=False)
    df = df[df["rank"] <= 10].sort_values(by=["date", "rank"])
    df["rank"] = df["rank"].astype(str)
    w = pd.pivot(data=df, index="date", columns="rank", values="f")
    w = w.div(w.sum(axis=1), axis=0)
    res = [pd.pivot(data=df, index="date", columns="rank", values=rt).mul(w).sum(axis=1)
           for rt in RETURNS]
    return pd.concat(res, axis=1).to_numpy()


# ---- ingest inputs ---------------------------------------------------------------------------------
SENTINEL = -7.25                                       # what absent / out-of-range cells hold


def ffill_inputs(seed=41, K=2, T=197, lda=64):
    """planes [K][T][lda] (absent cells SENTINEL), present [T][lda]: asset 0 a leading NaN run;
    asset 1 NaN runs across days 63/64 and 127/128; asset 2 never present; asset 3 one present
    day; asset 4 present days on both sides of an empty presence word; the rest random."""
    rng = np.random.default_rng(seed)
    present = rng.random((T, lda)) < 0.7
    planes = mixed_scale(rng, (K, T, lda))
    planes[rng.random(planes.shape) < 0.4] = np.nan
    present[:, :2] = True
    planes[:, :10, 0] = np.nan
    planes[0, 59, 1] = 3.5
    planes[:, 60:70, 1] = np.nan
    planes[1, 119, 1] = -0.0
    planes[:, 120:136, 1] = np.nan
    present[:, 2:5] = False
    present[100, 3] = True
    planes[:, 100, 3] = [np.nan, 2.0]
    present[[5, 63, 192, 196], 4] = True
    planes[:, [5, 63, 192, 196], 4] = [[1.0, np.nan, np.nan, 4.0], [np.nan, 2.0, np.nan, np.nan]]
    planes[:, ~present] = SENTINEL
    return planes, present


def date_fill_inputs(A: int, lda: int, seed=43):
    """planes [2][6][lda], present [6][lda]: 0, 1, 8192, 8193, about 20000 and all A rows per date;
    (date 2, column 0) has no NaN, (date 3, column 1) and (date 1, column 0) only NaN."""
    rng = np.random.default_rng(seed)
    counts = [0, 1, 8192, 8193, min(20000, A - 1), A]
    K, T = 2, len(counts)
    present = np.zeros((T, lda), dtype=bool)
    for t, c in enumerate(counts):
        present[t, rng.permutation(A)[:c]] = True
    planes = mixed_scale(rng, (K, T, lda))
    nan = rng.random(planes.shape) < 0.3
    nan[0, 2] = False
    nan[1, 3] = True
    nan[0, 1] = True
    nan[1, 1] = False
    planes[nan] = np.nan
    planes[:, ~present] = SENTINEL
    return planes, present


GROUP_SIZES = (0, 1, 7, 8, 129, 40, 8192, 8193, 20000, 65536)   # the 40-row group: all NaN


def group_inputs(seed=47):
    rng = np.random.default_rng(seed)
    offsets = np.r_[0, np.cumsum(GROUP_SIZES)].astype(np.int64)
    x = mixed_scale(rng, int(offsets[-1]))
    x[rng.random(len(x)) < 0.1] = np.nan
    x[offsets[1]] = 0.125                                  # the one-row group: a value
    x[offsets[5]:offsets[6]] = np.nan
    return x, offsets
