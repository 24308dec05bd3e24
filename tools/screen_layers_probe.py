"""Time the layers / long-short / top-k half of the factor screen on a stepped pipeline (default
config B's shape: 3,000 assets x 5,040 days; the train split, every feature, z on the fly):
``Pipeline.factor_screen()``, ``Pipeline.factor_screen(layers=True)`` and the only way to get the
same outputs without the batched kernels -- K sequential ``evaluate_grid`` calls, one per column,
on the same rows.  The three are run interleaved, round after round, in one process; each time is
a host clock around work that ends in a device synchronise.  Then the new entry points alone
(device events) with the layer kernel's algorithmic bytes -- K gathered planes plus the three
return planes per date -- against the HBM peak.
    python tools/screen_layers_probe.py [--assets 3000 --days 5040 --rounds 3]
One GPU; reads nothing outside the repository."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alpha-multi-factor-models_amd")]

HBM_TBS = 8.0                                                       # MI355X peak
LAYER_KEYS = ("layer_mean", "layer_cnt", "port", "cum_layer", "ls", "cum_port")


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, reps=5):
    import numpy as np
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    ts = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assets", type=int, default=3000)
    ap.add_argument("--days", type=int, default=5040)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import afm
    from afm.analyzer import evaluate_grid
    from afm.grid import unpack_bits
    from afm.pipeline import Pipeline
    from afm.synthetic import make_panel
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    pipe = Pipeline(afm.PanelGrid.from_panel(make_panel(a.assets, a.days, seed=2023,
                                                        tradable_p=0.9)))
    pipe.step()
    torch.cuda.synchronize()
    T, lda, nch, t1, K = pipe.T, pipe.lda, pipe.nch, pipe.sp.tr1, pipe.p
    print(f"{torch.cuda.get_device_name(0)}; train split {t1} dates x {lda} (A = {pipe.A}), "
          f"K = {K} columns, z on the fly", flush=True)

    # the rows of factor_screen(split='train', z=True), for the per-column loop
    call = pipe.ctx.call
    pipe.ctx.bind_stream()
    rb, pb = torch.zeros_like(pipe.zrows), torch.zeros_like(pipe.alldf)
    call("afm_row_bits", nch, lda, pipe.zrows, None, None, 0, t1, rb)
    call("afm_row_bits", nch, lda, pipe.alldf, None, None, 0, t1, pb)
    w1 = (t1 + 63) // 64
    rowm = unpack_bits(rb[:w1], t1)
    close, pbits = pipe.full.close[:t1], pb[:w1]
    years = (np.asarray(pipe.full.dates).astype("datetime64[Y]").astype(np.int64) + 1970)[:t1]
    nan = torch.full((t1, lda), float("nan"), dtype=torch.float64, device=rowm.device)

    def loop(keep=None):
        for k in range(K):
            c = int(pipe.feat[k].item())
            z = (pipe.out[c, :t1] - pipe.zs[k, :, 0]) * pipe.zs[k, :, 1]
            one = evaluate_grid(torch.where(rowm, z, nan), close, pbits, A=pipe.A, year=years)
            if keep is not None and k in keep:
                keep[k] = {key: one[key].cpu().numpy() for key in LAYER_KEYS}

    # warm every shape, and check the batched outputs against the loop's on a few columns
    pipe.factor_screen()
    got = pipe.factor_screen(layers=True)
    keep = {0: None, K // 2: None, K - 1: None}
    loop(keep)
    same = all(bool(((got[key][:, k] == v[key]) | (np.isnan(got[key][:, k].astype(np.float64)) &
                                                   np.isnan(v[key].astype(np.float64)))).all())
               for k, v in keep.items() for key in LAYER_KEYS)
    print(f"batched outputs of columns {sorted(keep)} bit-equal to the loop's: {same}", flush=True)

    ts = {"screen": [], "layers": [], "loop": []}
    for r in range(a.rounds):
        ts["screen"].append(wall_ms(lambda: pipe.factor_screen())[0])
        ts["layers"].append(wall_ms(lambda: pipe.factor_screen(layers=True))[0])
        ts["loop"].append(wall_ms(loop)[0])
        print(f"round {r}: factor_screen() {ts['screen'][-1]:.1f} ms, factor_screen(layers=True) "
              f"{ts['layers'][-1]:.1f} ms, {K} x evaluate_grid {ts['loop'][-1]:.1f} ms", flush=True)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    print(f"medians of {a.rounds}: factor_screen() {med['screen']:.1f} ms, "
          f"factor_screen(layers=True) {med['layers']:.1f} ms (+{med['layers'] - med['screen']:.1f}), "
          f"{K} x evaluate_grid {med['loop']:.1f} ms ({med['loop'] / K:.2f} ms per column): "
          f"the batched call is {med['loop'] / med['layers']:.1f}x faster", flush=True)

    # the new entry points alone, on the buffers factor_screen() left
    b = pipe._screen_bufs
    nd = len(got["dates_idx"])
    a0 = 0
    d_t = torch.from_numpy(np.ascontiguousarray(got["dates_idx"] - a0, dtype=np.int32)).to(rowm.device)
    cells = int(got["nrows"][got["dates_idx"]].sum())

    def layers():
        call("afm_screen_layers_f64", pipe.out[0, :t1], T * lda, t1, lda, pipe.feat, K, pipe.zs,
             None, d_t, nd, b["rows"], b["rows_idx"], b["nrows"], b["layer_mean"], b["layer_cnt"],
             b["port"], b["layers_scratch"])

    def series():
        call("afm_screen_layer_series_f64", nd, K, b["layer_mean"], b["port"], b["cum_layer"],
             b["ls"], b["cum_port"])
    ms_l, ms_s = event_ms(layers), event_ms(series)
    algo = cells * K * 8 + cells * 3 * 8
    items = nd * K
    print(f"afm_screen_layers_f64: {ms_l:.3f} ms for {nd} dates, {cells} rows "
          f"({cells / max(nd, 1):.0f} per date), {items} workgroups = "
          f"{ms_l * 1e3 / items * 256:.2f} us each on 256 CUs", flush=True)
    print(f"afm_screen_layers_f64 algorithmic bytes {algo / 1e9:.2f} GB (K gathered planes + 3 "
          f"return planes per date) -> {algo / ms_l / 1e9:.3f} TB/s, "
          f"{algo / ms_l / 1e9 / HBM_TBS:.1%} of {HBM_TBS} TB/s HBM", flush=True)
    chain = cells * K / 10.0                     # sequential Kahan steps of the longest-lived lanes
    print(f"layer-mean chains: {chain:.3g} sequential steps of one lane group per (date, column) "
          f"= {ms_l * 1e6 / chain * 256:.1f} ns of a CU per step if the chains were all of it",
          flush=True)
    print(f"afm_screen_layer_series_f64: {ms_s:.3f} ms for {nd} dates, K = {K}", flush=True)
    return 0 if same and med["layers"] < med["loop"] else 1


if __name__ == "__main__":
    sys.exit(main())
