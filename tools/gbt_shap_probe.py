"""Time the attribution of the boosted trees (afm.gbt, csrc/gbt_shap.hip) on a stepped pipeline
(default: the headline configuration, 10,000 assets x 5,040 days, the 97 z-scored features): a
fit of ``--rounds`` trees at depth 3 (the reference's model) and at depth 6, then

* the cover pass (afm_gbt_cover_i64) over the fit's resident bins and weights,
* the contributions of all trees on the test dates (afm_gbt_shap_f64 as Pipeline.gbt_contribs
  calls it): the per-date aggregates alone, and with the planes [nt][p+1][lda] as well.

Device events, median of ``--reps`` with [min, max] after a warm-up call.  Nothing is gated on these
numbers: there is no earlier implementation to compare with.  Results with the device name go to
profiles/gbt_shap.json.
    python tools/gbt_shap_probe.py [--assets 10000 --days 5040 --rounds 400 --reps 5 --out PATH]
One GPU; reads nothing outside the repository."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alpha-multi-factor-models_amd")]


def event_stats(fn, reps):
    """{median, min, max} ms of ``fn`` by device events, after one warm-up call."""
    import numpy as np
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assets", type=int, default=10000)
    ap.add_argument("--days", type=int, default=5040)
    ap.add_argument("--rounds", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depths", type=int, nargs="+", default=[3, 6])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gbt_shap.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import afm
    from afm.gbt import GBTParams, check_cover, shap_device
    from afm.pipeline import Pipeline
    from afm.synthetic import make_panel
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    pipe = Pipeline(afm.PanelGrid.from_panel(make_panel(a.assets, a.days, seed=2023,
                                                        tradable_p=0.9)))
    pipe.step()
    torch.cuda.synchronize()
    T, lda, p, sp = pipe.T, pipe.lda, pipe.p, pipe.sp
    nt = T - sp.s0
    res = {"device": torch.cuda.get_device_name(0), "assets": a.assets, "days": a.days,
           "reps": a.reps, "rounds": a.rounds, "p": p, "lda": lda, "test_dates": nt,
           "contrib_bytes": nt * (p + 1) * lda * 8,
           "note": "first measurement of new code: no parent time, nothing is gated on it",
           "depths": {}}
    print(json.dumps({k: v for k, v in res.items() if k != "depths"}), flush=True)
    call = pipe.ctx.call
    for D in a.depths:
        model = pipe.gbt_fit(GBTParams(n_rounds=a.rounds, max_depth=D), rows="train")
        torch.cuda.synchronize()
        check_cover(model)
        g = pipe.gbt
        n = int(g["rows_t"].numel())
        n_pad = int(g["bins"].shape[1])
        leaves = int((model.feat == -1).sum())
        r = {"rows": n, "train_rows": int((g["w"] > 0).sum().item()), "leaves": leaves,
             "splits": int((model.feat >= 0).sum())}
        print(f"depth {D}: {a.rounds} trees, {leaves} leaves, {r['splits']} splits", flush=True)
        pipe.ctx.bind_stream()
        cover = torch.empty_like(g["cover"])
        r["cover"] = event_stats(lambda: call("afm_gbt_cover_i64", g["bins"], n, n_pad, p, g["w"],
                                              g["feat"], g["bin"], D, a.rounds, cover), a.reps)
        assert torch.equal(cover, g["cover"])
        print(f"  cover pass over {n} rows: {r['cover']}", flush=True)
        outs = {}
        for name, planes in (("agg", False), ("agg_and_contrib", True)):
            def run():
                outs[name] = shap_device(pipe.ctx, model, a.rounds, pipe.out, T * lda, lda, sp.s0,
                                         nt, pipe.feat, p, pipe.zs, pipe.zrows, contrib=planes,
                                         agg=True)
            r[name] = event_stats(run, a.reps)
            print(f"  contributions on {nt} test dates ({name}): {r[name]}", flush=True)
        cells = int(outs["agg"]["cnt"].sum().item())
        r["cells"] = cells
        r["ns_per_cell_tree"] = r["agg"]["median_ms"] * 1e6 / max(cells * a.rounds, 1)
        assert torch.equal(outs["agg"]["agg"], outs["agg_and_contrib"]["agg"])
        # efficiency on the device: the rows of the planes sum to gbt_predict's plane
        c = outs["agg_and_contrib"]["contrib"]
        pred = pipe.gbt_predict(model)[sp.s0:]
        gap = (c.sum(dim=1) - pred).abs()
        r["max_row_sum_gap"] = float(gap[~torch.isnan(gap)].max().item())
        print(f"  {cells} cells, {r['ns_per_cell_tree']:.4f} ns per (cell, tree); "
              f"max |sum phi + bias - prediction| = {r['max_row_sum_gap']:.3e}", flush=True)
        del outs, c, pred, gap
        res["depths"][str(D)] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
