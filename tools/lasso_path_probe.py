#!/usr/bin/env python3
"""Time the batched Lasso solver against what a loop over afm_lasso_fit_f64 costs, on the
10,000 x 5,040 pipeline after one step(), with a 100-alpha scikit-learn-style grid on the train
Gram (headline design and the dense variant without tmr_ret1d).  Device events, median of
`reps` runs each:

* seq_ms        100 sequential afm_lasso_fit_f64 calls (one launch per alpha)
* batch_ms      one afm_lasso_batch_f64(warm=0) launch: 100 workgroups
* chain_ms      one afm_lasso_batch_f64(warm=1) launch: one workgroup walking the grid
* slowest_ms    the slowest single fit of the grid (batch_over_slowest = batch_ms / slowest_ms)
* lasso_cv_ms   the whole Pipeline.lasso_cv() (host wall time, synchronised), beside step_ms

Writes profiles/lasso_path.json (or the path given as the third argument).
usage: lasso_path_probe.py [assets=10000] [reps=11] [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alpha-multi-factor-models_amd"))


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    from dataclasses import replace

    import numpy as np
    import torch
    import afm
    from afm import _lib
    from afm.pipeline import DENSE_FEATURES, Pipeline, PipelineConfig
    from afm.regression import lasso_batch
    from afm.synthetic import make_panel
    A = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    reps = max(10, int(sys.argv[2]) if len(sys.argv) > 2 else 11)
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles",
                                                                  "lasso_path.json")
    torch.cuda.set_device(0)
    grid = afm.PanelGrid.from_panel(make_panel(A, 5040, seed=2023))
    L, P = _lib.lib(), _lib.ptr

    def events(fn):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return median(ts)

    def wall(fn):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return median(ts)

    result = {"device": torch.cuda.get_device_name(0), "assets": A, "days": 5040, "reps": reps,
              "n_alphas": 100, "configs": {}}
    base = PipelineConfig()
    for name, cfg in (("headline", base), ("dense", replace(base, features=DENSE_FEATURES))):
        pipe = Pipeline(grid, cfg)
        pipe.step()
        torch.cuda.synchronize()
        res = pipe.lasso_cv(n_alphas=100)
        p, c = pipe.p, pipe.cfg
        g, s = pipe._cv_gram[0:1], pipe.pool_s
        alphas = res["alphas"]
        a_dev = torch.from_numpy(alphas).cuda()
        beta = torch.empty((100, p + 1), dtype=torch.float64, device="cuda")
        info = torch.empty((100, 3), dtype=torch.float64, device="cuda")

        def fit(i):
            _lib.check(L.afm_lasso_fit_f64(pipe.ctx.bind_stream(), P(g), P(s), p,
                                           float(alphas[i]), c.max_iter, c.lasso_tol, 0,
                                           P(beta[i]), P(info[i])), "lasso")

        def seq():
            for i in range(100):
                fit(i)

        def batch(warm):
            return lasso_batch(g, s, p, a_dev, nprob=1, warm=warm, max_iter=c.max_iter,
                               tol=c.lasso_tol)

        seq_ms = events(seq)
        cold, cold_info = batch(False)
        assert cold[0].cpu().numpy().tobytes() == beta.cpu().numpy().tobytes()
        batch_ms = events(lambda: batch(False))
        chain_ms = events(lambda: batch(True))
        single = [events(lambda i=i: fit(i)) for i in range(100)]
        slowest = int(np.argmax(single))
        r = {"p": p, "n_train": res["n_train"], "n_valid": res["n_valid"],
             "seq_ms": seq_ms, "batch_ms": batch_ms, "chain_ms": chain_ms,
             "slowest_ms": single[slowest], "slowest_alpha_index": slowest,
             "batch_over_slowest": batch_ms / single[slowest],
             "seq_over_batch": seq_ms / batch_ms,
             "sweeps_cold": int(cold_info[0, :, 2].sum().item()),
             "sweeps_chain": int(res["n_iter"].sum()),
             "lasso_cv_ms": wall(lambda: pipe.lasso_cv(n_alphas=100)),
             "step_ms": wall(pipe.step),
             "best": res["best"], "alpha_": res["alpha_"],
             "nnz_at_best": int((res["coefs"][res["best"], 1:] != 0).sum()),
             "ic_valid_at_best": float(res["ic_valid"][res["best"]])}
        result["configs"][name] = r
        print(name, json.dumps(r), flush=True)
        del pipe
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
