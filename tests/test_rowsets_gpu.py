"""The row-set kernels -- afm_labels_f64, afm_drop_last_obs_bits(_range), afm_row_bits -- on
presence patterns built around the 64-day words: never present, a single day, only day 0, only
day T-1, bit 63 of word 0 with bit 0 of word 1, two days separated by two empty words, dense and
random (tests/ols_ref.py: presence).  Every result is compared word for word / bit for bit with
the Python-int references, and buffers are prefilled with sentinels so that a write outside the
requested range shows."""
import numpy as np
import pytest

import ols_ref as R

pytestmark = pytest.mark.gpu

SENT_A = 0x7FF8DEAD0000BEEF          # NaN payloads no kernel writes
SENT_B = 0x7FF8FACE0000F00D
SENT_W = 0x5A5AA5A5C3C33C3C
LDAS = [64, 320]                     # 320 reaches a second 256-thread block
TS = [1, 63, 64, 65, 130, 200]


def _assets(lda):
    return 40 if lda == 64 else 300  # patterns land in both thread blocks; the rest is padding


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _cuda(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _handle():
    from afm import _lib
    return _lib.lib(), _lib.ptr, _lib.Context.get(0).bind_stream(), _lib.check


def _words(t):
    return t.cpu().numpy().view(np.uint64)


# ---- afm_labels_f64 -----------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("lda", LDAS)
def test_labels(lda, T):
    import torch
    L, P, h, chk = _handle()
    rng = np.random.default_rng([47, lda, T])
    v = R.presence(T, lda, _assets(lda))
    excess, ret1d = rng.normal(size=(T, lda)), rng.normal(size=(T, lda))
    d_e, d_r, d_v = _cuda(excess), _cuda(ret1d), _cuda(R.pack_words(v))
    s_a = np.full((T, lda), SENT_A, dtype=np.int64).view(np.float64)
    s_b = np.full((T, lda), SENT_B, dtype=np.int64).view(np.float64)
    ranges = [(0, T), (5, 70), (63, 65), (64, 128), (T - 1, T), (-3, T + 9), (10, 10)]
    for t0, t1 in ranges:
        d_tg, d_tm = _cuda(s_a), _cuda(s_b)
        chk(L.afm_labels_f64(h, T, lda, t0, t1, P(d_e), P(d_r), P(d_v), P(d_tg), P(d_tm)),
            "afm_labels_f64")
        torch.cuda.synchronize()
        tg, tm = R.labels_ref(excess, ret1d, v, t0, t1, s_a, s_b)
        # (np.nan is the kernel's quiet-NaN pattern, R.NAN_BITS; everything else is a copy)
        assert (_bits(d_tg.cpu().numpy()) == _bits(tg)).all(), (lda, T, t0, t1, "target")
        assert (_bits(d_tm.cpu().numpy()) == _bits(tm)).all(), (lda, T, t0, t1, "tmr_ret1d")


def test_labels_equal_the_factor_panel_label_planes():
    """afm_labels_f64 == planes 96-97 of afm_factors_f64 on the present cells of a small panel."""
    import torch
    import afm
    from afm.synthetic import make_panel
    L, P, h, chk = _handle()
    p = make_panel(70, 150, seed=5, edge_cases=True, hole_frac=0.02)
    grid = afm.PanelGrid.from_panel(p)
    out, _ = afm.factor_panel(grid)
    T, lda = grid.T, grid.lda
    tg = torch.full((T, lda), 3.0, dtype=torch.float64, device="cuda")
    tm = torch.full((T, lda), 3.0, dtype=torch.float64, device="cuda")
    chk(L.afm_labels_f64(h, T, lda, 0, T, P(grid.excess), P(grid.ret1d), P(grid.vbits), P(tg),
                         P(tm)), "afm_labels_f64")
    torch.cuda.synchronize()
    v = grid.valid.cpu().numpy()
    assert v.sum() > 1000
    for plane, got in ((96, tg), (97, tm)):
        a, b = out[plane].cpu().numpy()[v], got.cpu().numpy()[v]
        assert ((a == b) | (np.isnan(a) & np.isnan(b))).all()
        assert np.isnan(b).sum() >= (v.sum(axis=0) > 0).sum()    # every asset's last day is NaN
    assert (tg.cpu().numpy()[~v] == 3.0).all() and (tm.cpu().numpy()[~v] == 3.0).all()


# ---- afm_drop_last_obs_bits, afm_drop_last_obs_bits_range ---------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("lda", LDAS)
def test_drop_last_obs_bits(lda, T):
    """in_bits is random (not a subset of presence: the bit of the last present day is set for
    some assets and clear for others).  The last day comes from all T dates even when it lies
    outside the range; words outside the range keep the sentinel."""
    import torch
    L, P, h, chk = _handle()
    rng = np.random.default_rng([53, lda, T])
    v = R.presence(T, lda, _assets(lda))
    vw = R.pack_words(v)
    nch = vw.shape[0]
    inw = rng.integers(0, 2 ** 64, size=vw.shape, dtype=np.uint64)
    sent = np.full(vw.shape, SENT_W, dtype=np.uint64)
    d_v, d_in = _cuda(vw), _cuda(inw)
    d_out = _cuda(sent)
    chk(L.afm_drop_last_obs_bits(h, T, lda, P(d_v), P(d_in), P(d_out)), "drop_last_obs_bits")
    torch.cuda.synchronize()
    whole = _words(d_out)
    ref = R.drop_last_ref(vw, inw, sent, 0, nch)
    # the last-day bit was set in some columns and clear in others
    changed = (ref != inw).any(axis=0)
    assert changed.any() and (~changed[v.any(axis=0)]).any()
    assert (whole == ref).all()
    if T != 200:
        return
    for t0, t1 in [(0, 64), (64, 200), (128, 200), (0, 200)]:
        d_out = _cuda(sent)
        chk(L.afm_drop_last_obs_bits_range(h, T, lda, P(d_v), P(d_in), P(d_out), t0, t1),
            "drop_last_obs_bits_range")
        torch.cuda.synchronize()
        got = _words(d_out)
        c0, c1 = t0 // 64, (t1 + 63) // 64
        assert (got == R.drop_last_ref(vw, inw, sent, c0, c1)).all(), (t0, t1)
        assert (got[c0:c1] == whole[c0:c1]).all()                # the concatenation of ranges
        assert (np.delete(got, np.s_[c0:c1], axis=0) == SENT_W).all()


# ---- afm_row_bits -------------------------------------------------------------------------------
def _row_ranges(nch):
    full = 64 * nch
    rs = [(0, full)]
    rs += [(t0, full) for t0 in (1, 63, 64, 65, 130)]
    rs += [(0, t1) for t1 in (1, 63, 64, 65, 128, 129)]
    rs += [(63, 65), (65, 129), (64, 128), (70, 70), (0, 0), (100, 30), (full, full + 5)]
    return rs


@pytest.mark.parametrize("masks", ["a", "a_b", "a_ok", "a_b_ok"])
@pytest.mark.parametrize("nch", [1, 2, 4])
@pytest.mark.parametrize("lda", LDAS)
def test_row_bits(lda, nch, masks):
    """Covers a word cleared because t0 - d0 >= 64, one cleared because t1 <= d0, and t1 - d0 ==
    64 exactly (no shift by 64)."""
    import torch
    L, P, h, chk = _handle()
    rng = np.random.default_rng([59, lda, nch, len(masks)])
    a = rng.integers(0, 2 ** 64, size=(nch, lda), dtype=np.uint64)
    b = rng.integers(0, 2 ** 64, size=(nch, lda), dtype=np.uint64) if "_b" in masks else None
    ok = (rng.random(lda) < 0.8).astype(np.int32) if "_ok" in masks else None
    d_a = _cuda(a)
    d_b = _cuda(b) if b is not None else None
    d_ok = _cuda(ok) if ok is not None else None
    for t0, t1 in _row_ranges(nch):
        d_out = _cuda(np.full((nch, lda), SENT_W, dtype=np.uint64))
        chk(L.afm_row_bits(h, nch, lda, P(d_a), P(d_b) if d_b is not None else None,
                           P(d_ok) if d_ok is not None else None, t0, t1, P(d_out)),
            "afm_row_bits")
        torch.cuda.synchronize()
        assert (_words(d_out) == R.row_bits_ref(a, b, ok, t0, t1)).all(), (lda, nch, masks, t0, t1)
