"""Time the boosted trees (afm.gbt, csrc/gbt.hip) on a stepped pipeline (default: the headline
configuration, 10,000 assets x 5,040 days, the 97 z-scored features, train rows weight 1 and valid
rows weight 0): the cuts (values + sort per column, host clock), the binning, one histogram level
at depths 0, 1 and 2 on the rows' nodes of the first tree, and a whole round (the difference of a
3-round and a 1-round fit, halved).  Device events, median of ``--reps`` after a warm-up call.

The histogram kernel's algorithmic bytes -- per row 16 B of (node, q, w) for every (column tile,
node group) pass and one byte per column -- are given per second and as a share of the HBM figure
bench.py uses for the factor kernel (8 TB/s); also under three forced row chunks
("gbt_rows_per_wg"), whose histograms must be the same bits.  Results with the device name go to
profiles/gbt.json.
    python tools/gbt_probe.py [--assets 10000 --days 5040 --reps 5 --max-bin 256 --out PATH]
One GPU; reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alpha-multi-factor-models_amd"),
                os.path.join(ROOT, "tools")]

HBM_PEAK = 8.0e12              # bench.py's HBM_PEAK_GBS
PAIRS = 16                     # (node, column) pairs of a histogram workgroup (csrc/gbt.hip)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assets", type=int, default=10000)
    ap.add_argument("--days", type=int, default=5040)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-bin", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbt.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import afm
    from afm import _lib
    from afm.factors import TARGET
    from afm.gbt import GBTParams, device_cuts
    from afm.pipeline import Pipeline
    from afm.synthetic import make_panel
    from screen_layers_probe import event_ms
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    B, D = a.max_bin, 3
    pipe = Pipeline(afm.PanelGrid.from_panel(make_panel(a.assets, a.days, seed=2023,
                                                        tradable_p=0.9)))
    pipe.step()
    torch.cuda.synchronize()
    dev, T, lda, p, sp = pipe.out.device, pipe.T, pipe.lda, pipe.p, pipe.sp
    call = pipe.ctx.call
    pipe.ctx.bind_stream()
    rt, ra = pipe._gbt_rows(sp.v1)
    n = int(rt.numel())
    n_pad = (n + 63) // 64 * 64
    w = (rt < sp.tr1).to(torch.int32)
    y = torch.empty(n, dtype=torch.float64, device=dev)
    call("afm_gbt_values_f64", pipe.out, T * lda, T, lda,
         torch.tensor([TARGET], dtype=torch.int32, device=dev), 0, None, rt, ra, n, y)
    res = {"device": torch.cuda.get_device_name(0), "assets": a.assets, "days": a.days,
           "reps": a.reps, "rows": n, "train_rows": int((w > 0).sum().item()), "p": p,
           "max_bin": B, "max_depth": D}
    print(json.dumps(res), flush=True)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cuts, ncuts = device_cuts(pipe.out, pipe.feat, w, T=T, lda=lda, col_stride=T * lda, zs=pipe.zs,
                              rows_t=rt, rows_a=ra, n=n, max_bin=B)
    torch.cuda.synchronize()
    res["cuts_ms"] = (time.perf_counter() - t0) * 1e3
    bins = torch.empty((p, n_pad), dtype=torch.uint8, device=dev)

    def run_bin():
        call("afm_gbt_bin_f64", pipe.out, T * lda, T, lda, pipe.feat, p, pipe.zs, rt, ra, n, n_pad,
             cuts, ncuts, B, bins)
    res["bin_ms"] = event_ms(run_bin, reps=a.reps)
    res["bin_gbs"] = n * p * (8 + 1) / res["bin_ms"] / 1e6          # a double in, a byte out
    print(f"cuts {res['cuts_ms']:.0f} ms (host clock), binning {res['bin_ms']:.2f} ms "
          f"({res['bin_gbs']:.0f} GB/s of values + bins)", flush=True)

    def fit(rounds):
        prm = GBTParams(n_rounds=rounds, max_depth=D, max_bin=B)
        nn = prm.n_nodes
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        out = [torch.empty((rounds, nn), **i32), torch.empty((rounds, nn), **i32),
               torch.empty((rounds, nn), **f64), torch.empty((rounds, nn), **f64)]
        F, ev = torch.zeros(n, **f64), torch.empty((rounds, 2, 6), **f64)

        def run():
            F.zero_()
            call("afm_gbt_fit_f64", bins, n, n_pad, p, cuts, ncuts, y, w, rounds, D, B, prm.eta,
                 prm.reg_lambda, prm.gamma, prm.min_child_weight, *out, F, ev, scr)
        return run, out
    scr = torch.empty(call("afm_gbt_scratch_bytes", n, p, D, B) // 8, dtype=torch.int64,
                      device=dev)
    run1, trees = fit(1)
    run3, _ = fit(3)
    ms1, ms3 = event_ms(run1, reps=a.reps), event_ms(run3, reps=a.reps)
    res.update(fit1_ms=ms1, fit3_ms=ms3, round_ms=(ms3 - ms1) / 2)
    print(f"fit of 1 round {ms1:.2f} ms, of 3 rounds {ms3:.2f} ms -> {res['round_ms']:.2f} ms per "
          f"round (depth {D})", flush=True)

    # the first round's gradients and the rows' nodes of the first tree, level by level
    g = -y
    gmax = float(g[w > 0].abs().max().item())
    import math
    e = min(62 - int(w.sum().item()).bit_length() - math.frexp(gmax)[1], 960) if gmax else 0
    q = torch.round(g * math.ldexp(1.0, e)).to(torch.int64) * w
    feat, sbin = trees[0][0].long(), trees[1][0].long()
    node = torch.zeros(n, dtype=torch.int64, device=dev)
    rows = torch.arange(n, device=dev)
    res["hist"] = {}
    for d in range(D):
        nnodes, first = 1 << d, (1 << d) - 1
        nd32 = node.to(torch.int32)
        hist = torch.empty((nnodes, p, B, 2), dtype=torch.int64, device=dev)
        nn = min(nnodes, PAIRS)
        passes = -(-p // (PAIRS // nn)) * -(-nnodes // nn)
        nbytes = n * (16 * passes + p)
        r = {"nnodes": nnodes, "passes": passes, "bytes": nbytes}
        same = None
        for opt in (0, 16384, 65536, 1 << 20):
            with _lib.options(gbt_rows_per_wg=opt):
                ms = event_ms(lambda: call("afm_gbt_hist_i64", bins, n, n_pad, p, B, nd32, q, w,
                                           nnodes, hist), reps=a.reps)
            bits = hist.cpu().numpy().tobytes()
            assert same is None or bits == same, "the work split changed the histogram"
            same = bits
            r[f"ms_rows_{opt}"] = ms
        r["ms"] = r["ms_rows_0"]
        r["tbs"] = nbytes / r["ms"] / 1e9
        r["hbm_frac"] = nbytes / (r["ms"] * 1e-3) / HBM_PEAK
        r["lds_adds_per_ns"] = 2 * int((w > 0).sum().item()) * p / (r["ms"] * 1e6)
        res["hist"][f"depth{d}"] = r
        print(f"hist depth {d}: {nnodes} nodes, {passes} passes, {r['ms']:.2f} ms "
              f"({nbytes / 1e9:.1f} GB: {r['tbs']:.2f} TB/s = {r['hbm_frac']:.3f} of HBM peak; "
              f"{r['lds_adds_per_ns']:.1f} LDS adds per ns); chunks of 16384 rows "
              f"{r['ms_rows_16384']:.2f} ms, of 65536 {r['ms_rows_65536']:.2f} ms, of 2^20 rows "
              f"{r[f'ms_rows_{1 << 20}']:.2f} ms",
              flush=True)
        v = first + node.clamp(min=0)
        k = feat[v]
        go = (node >= 0) & (k >= 0)                       # a row of a leaf is in no later level
        right = bins[k.clamp(min=0), rows].long() > sbin[v]
        node = torch.where(go, 2 * node + right.long(), torch.full_like(node, -1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
