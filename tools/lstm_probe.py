"""Time the stacked LSTM ensembles (afm.lstm, csrc/lstm.hip): one batch step -- the forward, backward
and gradient / Adam kernels of afm_lstm_grad_f64's and afm_lstm_fit_f64's launches -- at the
reference's shape (T = 98, d = 1, hidden 100 / 100, batches of 256 rows) for M = 1 and 8 models, and
at a window shape (T = 20, d = 29, hidden 128 / 64); and the forward pass over 16,384 rows.  A
synthetic standard-normal design (the time of a step does not depend on the values); device events,
``--reps`` timed runs after a warm-up, the median with the minimum and the maximum.  The fit of
``--steps`` steps gives the step time; the gradient call next to the forward call over the same
batch gives the split: forward, and backward + gradient tiles.  Reported with the fraction of the
fp64 MFMA peak (78.6 TF/s) that 3 * 2 * rows * T * ((d + H1) 4 H1 + (H1 + H2) 4 H2) flop in the
step's time come to.  Results with the device name go to profiles/lstm.json.
    python tools/lstm_probe.py [--steps 8 --reps 5 --out PATH]
One GPU; reads nothing outside the repository."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "alpha-multi-factor-models_amd")]

PEAK = 78.6e12


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
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from afm import _lib
    from afm.lstm import lstm_init, param_count
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    f64 = dict(dtype=torch.float64, device="cuda")
    ctx = _lib.Context.get(0)
    ctx.bind_stream()
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "reps": a.reps,
           "peak_fp64_mfma_flops": PEAK, "cases": []}
    batch, fwd_rows = 256, 16384
    for T, d, h1, h2, M in ((98, 1, 100, 100, 1), (98, 1, 100, 100, 8), (20, 29, 128, 64, 1)):
        n = max(a.steps * batch, fwd_rows)
        P = param_count(d, h1, h2)
        gen = torch.Generator(device="cuda").manual_seed(1)
        X = torch.randn((T, d, n), generator=gen, **f64)
        y = 0.1 * torch.randn(n, generator=gen, **f64)
        theta0 = torch.from_numpy(np.stack([lstm_init(d, (h1, h2), s) for s in range(M)])).cuda()
        theta = theta0.clone()
        evals = torch.empty((M, 1, 2, 6), **f64)
        scr = torch.empty(ctx.call("afm_lstm_scratch_bytes", T, d, h1, h2, M, batch) // 8, **f64)
        lr = (ctypes.c_double * M)(*([1e-3] * M))
        grad = torch.empty((M, P), **f64)
        out = torch.empty((M, n), **f64)

        def fit():
            theta.copy_(theta0)
            ctx.call("afm_lstm_fit_f64", X, y, n, a.steps * batch, 0, T, d, h1, h2, M, theta, lr,
                     0.9, 0.999, 1e-7, batch, 1, evals, None, scr)

        def gradient():
            ctx.call("afm_lstm_grad_f64", X, y, n, 0, batch, T, d, h1, h2, M, theta0, grad, None,
                     scr)

        def forward_batch():
            ctx.call("afm_lstm_forward_f64", X, n, 0, batch, T, d, h1, h2, M, theta0, out)

        def forward():
            ctx.call("afm_lstm_forward_f64", X, n, 0, fwd_rows, T, d, h1, h2, M, theta0, out)
        med, lo, hi = event_stats(fit, a.reps)
        gmed, glo, ghi = event_stats(gradient, a.reps)
        bmed, blo, bhi = event_stats(forward_batch, a.reps)
        fmed, flo, fhi = event_stats(forward, a.reps)
        flop = 3 * 2 * batch * T * ((d + h1) * 4 * h1 + (h1 + h2) * 4 * h2) * M
        step = med / a.steps
        r = {"T": T, "d": d, "hidden": [h1, h2], "M": M, "batch": batch, "params": P,
             "fit_ms": med, "fit_ms_min": lo, "fit_ms_max": hi, "ms_per_step": step,
             "grad_call_ms": gmed, "grad_call_ms_min": glo, "grad_call_ms_max": ghi,
             "forward_batch_ms": bmed, "forward_batch_ms_min": blo, "forward_batch_ms_max": bhi,
             "backward_and_tiles_ms": gmed - bmed,
             "step_gflop": flop / 1e9, "fraction_of_peak": flop / (step * 1e-3) / PEAK,
             "forward_rows": fwd_rows, "forward_ms": fmed, "forward_ms_min": flo,
             "forward_ms_max": fhi, "forward_rows_per_s": M * fwd_rows / (fmed * 1e-3)}
        res["cases"].append(r)
        print(f"T = {T}, d = {d}, hidden {h1}/{h2}, M = {M}: {step:.3f} ms per step "
              f"[fit of {a.steps}: {lo:.2f}..{hi:.2f} ms]; one gradient call {gmed:.3f} ms, of it the "
              f"forward kernel alone {bmed:.3f} ms; {flop / 1e9:.1f} GFLOP a step = "
              f"{100 * r['fraction_of_peak']:.2f} % of the fp64 MFMA peak; forward of {fwd_rows} "
              f"rows {fmed:.2f} ms [{flo:.2f}, {fhi:.2f}]", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
