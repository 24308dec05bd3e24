"""Time the network ensembles (afm.mlp, csrc/mlp.hip) at the reference's shape: 29 inputs, hidden
widths 128 and 32, batches of 256 rows, for M = 1, 16 and 256 models side by side (one workgroup
each).  A fit of ``--steps`` batch steps on a synthetic standard-normal design (the time of a step
does not depend on the values) runs as one launch; device events, ``--reps`` timed runs after a
warm-up, the median with the minimum and the maximum.  Reported per M: microseconds per batch step
and model-steps per second; and how far a step of M = 256 is from a step of M = 1 -- what sharing
L2 and HBM among 256 workgroups costs.  The forward kernel over the same rows is timed beside it.
Results with the device name go to profiles/mlp.json.
    python tools/mlp_probe.py [--steps 64 --reps 5 --models 1 16 256 --out PATH]
One GPU; reads nothing outside the repository."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alpha-multi-factor-models_amd")]


def event_stats(fn, reps):
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from afm import _lib
    from afm.mlp import glorot_init, param_count
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    p, h1, h2, batch = 29, 128, 32, 256
    n = a.steps * batch
    P = param_count(p, h1, h2)
    f64 = dict(dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((p, n), generator=gen, **f64)
    y = 0.1 * torch.randn(n, generator=gen, **f64)
    ctx = _lib.Context.get(0)
    ctx.bind_stream()
    res = {"device": torch.cuda.get_device_name(0), "p": p, "hidden": [h1, h2], "batch": batch,
           "steps": a.steps, "reps": a.reps, "params": P, "fits": {}}
    with _lib.options(mlp_steps_per_launch=1 << 20):              # one launch: no launch seams
        for M in a.models:
            theta0 = torch.from_numpy(np.stack([glorot_init(p, (h1, h2), s) for s in range(M)])).cuda()
            theta = theta0.clone()
            evals = torch.empty((M, 1, 2, 6), **f64)
            scr = torch.empty(ctx.call("afm_mlp_scratch_bytes", p, h1, h2, M, batch) // 8, **f64)
            lr = (ctypes.c_double * M)(*([1e-4] * M))

            def fit():
                theta.copy_(theta0)
                ctx.call("afm_mlp_fit_f64", X, y, n, n, 0, p, h1, h2, M, theta, lr, 0.9, 0.999,
                         1e-7, batch, 1, evals, None, scr)
            out = torch.empty((M, n), **f64)

            def forward():
                ctx.call("afm_mlp_forward_f64", X, n, 0, n, p, h1, h2, M, theta, out)
            med, lo, hi = event_stats(fit, a.reps)
            fmed, flo, fhi = event_stats(forward, a.reps)
            r = {"fit_ms": med, "fit_ms_min": lo, "fit_ms_max": hi,
                 "us_per_step": med * 1e3 / a.steps, "us_per_step_min": lo * 1e3 / a.steps,
                 "us_per_step_max": hi * 1e3 / a.steps,
                 "model_steps_per_s": M * a.steps / (med * 1e-3),
                 "forward_ms": fmed, "forward_ms_min": flo, "forward_ms_max": fhi,
                 "forward_rows_per_s": M * n / (fmed * 1e-3)}
            res["fits"][str(M)] = r
            print(f"M = {M}: fit of {a.steps} steps {med:.2f} ms [{lo:.2f}, {hi:.2f}] -> "
                  f"{r['us_per_step']:.1f} us per step, {r['model_steps_per_s']:.3g} model-steps/s; "
                  f"forward of {n} rows {fmed:.3f} ms [{flo:.3f}, {fhi:.3f}]", flush=True)
    ms = [str(m) for m in a.models]
    if "1" in ms and len(ms) > 1:
        res["step_ratio_last_vs_1"] = (res["fits"][ms[-1]]["us_per_step"]
                                       / res["fits"]["1"]["us_per_step"])
        print(f"a step of M = {ms[-1]} takes {res['step_ratio_last_vs_1']:.2f} x a step of M = 1",
              flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
