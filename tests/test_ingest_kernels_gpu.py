"""The ingest kernels of csrc/analyzer.hip (ffill, per-date mean fill, per-group demean) called
directly on hand-built grids against the pandas / numpy statements of tests/analyzer_ref.py (pinned
on the CPU by tests/test_analyzer_ref.py).  Bit for bit, NaN equal to NaN; no tolerance."""
import numpy as np
import pytest

import analyzer_ref as R
from helpers import same

pytestmark = pytest.mark.gpu


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def run(name, *args):
    from afm import _lib
    return _lib.run(name, *args)


def test_ffill_presence_word_edges():
    """T = 197: a leading NaN run stays NaN; NaN runs across days 63/64 and 127/128; a value
    carried over an empty presence word; an asset never present and one present once; absent
    cells (a sentinel) are not written."""
    planes, present = R.ffill_inputs()
    K, T, lda = planes.shape
    got = dev(planes)
    run("afm_ffill_f64", K, T, lda, got, dev(R.pack_bits(present)))
    want = R.ffill_pandas(planes, present)
    assert same(got.cpu().numpy(), want)
    assert np.isnan(want[:, :10, 0]).all() and want[0, 69, 1] == 3.5 and want[0, 196, 4] == 4.0
    assert want[1, 196, 4] == 2.0 and np.isnan(want[0, 100, 3])
    assert (want[:, ~present] == R.SENTINEL).all()


@pytest.mark.parametrize("A,lda", [(65536, 65536), (20001, 20032)])
def test_date_mean_fill_buffered_means(A, lda):
    """Per-date column means over 0, 1, 8192, 8193, about 20000 and A present rows (65536 is the
    entry point's limit): past 8192 rows numpy's buffered reduction, not one pairwise tree.  A
    column without NaN is left as it is, an all-NaN column stays NaN, absent cells and the padding
    columns are not written."""
    import torch
    planes, present = R.date_fill_inputs(A, lda)
    K, T, _ = planes.shape
    got = dev(planes)
    run("afm_date_mean_fill_f64", K, T, A, lda, got, dev(R.pack_bits(present)),
        torch.empty_like(got))
    assert same(got.cpu().numpy(), R.date_mean_fill_ref(planes, present))


def test_date_mean_fill_rejects_more_than_65536_assets():
    import torch
    from afm._lib import AfmError
    A, lda = 65537, 65600
    planes = torch.full((1, 1, lda), float("nan"), dtype=torch.float64, device="cuda:0")
    bits = torch.full((1, lda), 1, dtype=torch.int64, device="cuda:0")
    with pytest.raises(AfmError, match=r"\(-1\)"):                      # AFM_E_ARG
        run("afm_date_mean_fill_f64", 1, 1, A, lda, planes, bits, torch.empty_like(planes))
    torch.cuda.synchronize()
    assert torch.isnan(planes).all()                                    # no launch


def test_group_demean_buffered_means():
    """Groups of 0, 1, 7, 8, 129, 8192, 8193, 20000 and 65536 rows (the limit) with about 10 % NaN
    and one all-NaN group (output all NaN): x - nanmean per group, past 8192 rows by numpy's
    buffered reduction."""
    import torch
    from afm._lib import AfmError
    x, off = R.group_inputs()
    xt = dev(x)
    out = torch.full_like(xt, R.SENTINEL)
    run("afm_group_demean_f64", len(off) - 1, dev(off), int(np.diff(off).max()), xt, out,
        torch.empty_like(xt))
    assert same(out.cpu().numpy(), R.group_demean_ref(x, off))
    out.fill_(R.SENTINEL)
    with pytest.raises(AfmError, match=r"\(-1\)"):                      # AFM_E_ARG
        run("afm_group_demean_f64", len(off) - 1, dev(off), 65537, xt, out, torch.empty_like(xt))
    torch.cuda.synchronize()
    assert (out == R.SENTINEL).all()                                    # no launch
