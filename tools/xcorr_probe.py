"""Time the cross-factor correlation of the factor screen on a stepped pipeline (default config
B's shape: 3,000 assets x 5,040 days; the train split, every feature, z on the fly): the two entry
points of include/afm_xcorr.h alone (device events, median of 5) on the buffers
``Pipeline.factor_screen(xcorr=True)`` left, with the algorithmic flops of the symmetric product
-- rows * K (K + 1) on the fast path, which the z rows (dropna rows) take -- against the fp64
matrix peak, and ``factor_screen()`` with and without ``xcorr`` (host clock, device synchronised).
A few dates are checked against numpy's corrcoef on the same values first.
    python tools/xcorr_probe.py [--assets 3000 --days 5040 --rounds 3]
One GPU; reads nothing outside the repository."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alpha-multi-factor-models_amd"),
                os.path.join(ROOT, "tools")]

F64_MATRIX_TFS = 78.6                                               # MI355X fp64 MFMA peak
POOLED_GRAM_FRACTION = 0.45                                         # the pooled Gram's, DESIGN.md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assets", type=int, default=3000)
    ap.add_argument("--days", type=int, default=5040)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import afm
    from afm.pipeline import Pipeline
    from afm.synthetic import make_panel
    from screen_layers_probe import event_ms, wall_ms
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    pipe = Pipeline(afm.PanelGrid.from_panel(make_panel(a.assets, a.days, seed=2023,
                                                        tradable_p=0.9)))
    pipe.step()
    torch.cuda.synchronize()
    T, lda, t1, K = pipe.T, pipe.lda, pipe.sp.tr1, pipe.p
    print(f"{torch.cuda.get_device_name(0)}; train split {t1} dates x {lda} (A = {pipe.A}), "
          f"K = {K} columns, z on the fly", flush=True)
    pipe.factor_screen()
    got = pipe.factor_screen(xcorr=True)
    nd = len(got["dates_idx"])
    rows = int(got["nrows"][got["dates_idx"]].sum())

    # a few dates against numpy on the same z values (the z rows have no missing cell)
    b = pipe._screen_bufs
    ridx = b["rows_idx"]
    worst = 0.0
    for i in np.linspace(0, nd - 1, 5).astype(int):
        t = int(got["dates_idx"][i])
        n = int(got["nrows"][t])
        idx = ridx[t, :n].long()
        z = (pipe.out[pipe.feat.long(), t][:, idx] - pipe.zs[:K, idx, 0]) * pipe.zs[:K, idx, 1]
        with np.errstate(all="ignore"):
            ref = np.corrcoef(z.cpu().numpy())
        x = got["xcorr_dev"][i].cpu().numpy()
        ok = ~np.isnan(x) & ~np.isnan(ref)
        worst = max(worst, float(np.abs(x[ok] - ref[ok]).max()))
    print(f"5 dates against numpy.corrcoef: largest difference {worst:.2e}", flush=True)

    ts = {"screen": [], "xcorr": []}
    for r in range(a.rounds):
        ts["screen"].append(wall_ms(lambda: pipe.factor_screen())[0])
        ts["xcorr"].append(wall_ms(lambda: pipe.factor_screen(xcorr=True))[0])
    med = {k: float(np.median(v)) for k, v in ts.items()}
    print(f"medians of {a.rounds}: factor_screen() {med['screen']:.1f} ms, "
          f"factor_screen(xcorr=True) {med['xcorr']:.1f} ms (+{med['xcorr'] - med['screen']:.1f})",
          flush=True)

    call = pipe.ctx.call
    pipe.ctx.bind_stream()
    d_t = torch.from_numpy(np.ascontiguousarray(got["dates_idx"], dtype=np.int32)).to(ridx.device)

    def xcorr():
        call("afm_screen_xcorr_f64", pipe.out[0, :t1], T * lda, t1, lda, pipe.feat, K, pipe.zs,
             None, d_t, nd, None, b["rows_idx"], b["nrows"], b["xcorr"])

    def summary():
        call("afm_screen_xcorr_summary_f64", b["xcorr"], nd, K, b["xcorr_stats"])
    ms_x, ms_s = event_ms(xcorr), event_ms(summary)
    flops = rows * K * (K + 1)
    frac = flops / (ms_x * 1e-3) / 1e12 / F64_MATRIX_TFS
    print(f"afm_screen_xcorr_f64: {ms_x:.3f} ms for {nd} dates, {rows} rows "
          f"({rows / max(nd, 1):.0f} per date), K = {K}; algorithmic flops rows K (K + 1) = "
          f"{flops / 1e9:.2f} G -> {flops / (ms_x * 1e-3) / 1e12:.2f} TF/s = {frac:.3f} of the "
          f"{F64_MATRIX_TFS} TF/s fp64 matrix peak (the pooled Gram: {POOLED_GRAM_FRACTION})",
          flush=True)
    print(f"afm_screen_xcorr_summary_f64: {ms_s:.3f} ms for {nd} dates, K = {K} "
          f"({nd * K * K * 8 / 1e6:.0f} MB read twice)", flush=True)
    return 0 if worst < 1e-9 else 1


if __name__ == "__main__":
    sys.exit(main())
