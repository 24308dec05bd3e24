"""The network kernels of csrc/mlp.hip against tests/mlp_ref.py: the forward values inside the
derived bound of their longdouble value, one Adam step on the exact grid bit for bit, whole
trajectories within the reference's own fp64-versus-longdouble spread, the invariances of the fit
(runs, steps per launch, ensemble composition, eval rows) bit for bit, and the argument rules."""
import ctypes

import numpy as np
import pytest

import mlp_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 16), (5, 16, 16), (29, 128, 32), (64, 128, 64)]


def planes(X, n_pad, y=None, poison=True):
    """device X [p][n_pad] (and y [n_pad]) with NaN / inf in every cell past the rows of X."""
    import torch
    n, p = X.shape
    Xp = np.full((p, n_pad), np.nan if poison else 0.0)
    Xp[:, n:][:, ::2] = np.inf if poison else 0.0
    Xp[:, :n] = X.T
    out = [torch.from_numpy(Xp).cuda()]
    if y is not None:
        yp = np.full(n_pad, np.nan if poison else 0.0)
        yp[:n] = y
        out.append(torch.from_numpy(yp).cuda())
    return out if y is not None else out[0]


def model(shape, n, seed, M=1):
    from afm.mlp import glorot_init
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, shape[0]))
    y = 0.1 * rng.standard_normal(n)
    theta = np.stack([glorot_init(shape[0], shape[1:], seed + m) for m in range(M)])
    theta += 0.05 * rng.standard_normal(theta.shape)
    return X, y, theta


def gpu_fit(X, y, n_train, n_eval, shape, theta0, lrs, batch, epochs, S=None, n_pad=None, **adam):
    """afm.mlp.fit_device on poisoned planes -> host (theta [M][P], evals, snaps)."""
    import torch
    from afm import _lib
    from afm.mlp import MLPParams, fit_device
    theta0 = np.atleast_2d(theta0)
    M = len(theta0)
    n_pad = n_pad or (len(y) + 63) // 64 * 64
    Xd, yd = planes(X[:n_train + n_eval], n_pad, y[:n_train + n_eval])
    prm = MLPParams(hidden=shape[1:], lr=tuple(np.broadcast_to(lrs, M).tolist()), epochs=epochs,
                    batch_size=batch, seeds=tuple(range(M)), **adam)
    if S is None:
        res = fit_device(Xd, yd, n_train, n_eval, prm, theta0=theta0)
    else:
        with _lib.options(mlp_steps_per_launch=S):
            res = fit_device(Xd, yd, n_train, n_eval, prm, theta0=theta0)
    torch.cuda.synchronize()
    return tuple(res[k].cpu().numpy() for k in ("theta", "evals", "snaps"))


# ---- forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_within_the_bound_and_slices_bitwise(shape):
    import torch
    from afm.mlp import forward_device
    n, n_pad, M = 200, 256, 2
    X, _, theta = model(shape, n, 3, M)
    Xd = planes(X, n_pad)
    th = torch.from_numpy(theta).cuda()
    out = torch.full((M, n_pad), -7.0, dtype=torch.float64, device="cuda")
    forward_device(Xd, th, shape[1:], 0, n, out=out)
    full = out.cpu().numpy()
    assert (full[:, n:] == -7.0).all() and np.isfinite(full[:, :n]).all()
    for m in range(M):
        f, E = R.forward_bound(theta[m], X, shape)
        err = np.abs(full[m, :n].astype(R.LD) - f)
        print(shape, m, "forward error / bound", float((err / E).max()))
        assert (err <= E).all()
    # a window that is no multiple of the tile, at an offset that is none either
    for i0, k in ((37, 101), (64, 64), (199, 1), (3, 13)):
        out = torch.full((M, n_pad), -7.0, dtype=torch.float64, device="cuda")
        forward_device(Xd, th, shape[1:], i0, k, out=out)
        part = out.cpu().numpy()
        assert part[:, i0:i0 + k].tobytes() == full[:, i0:i0 + k].tobytes()
        assert (part[:, :i0] == -7.0).all() and (part[:, i0 + k:] == -7.0).all()
    forward_device(Xd, th, shape[1:], 5, 0, out=out)          # n = 0: nothing
    assert out.cpu().numpy().tobytes() == part.tobytes()


def test_forward_over_many_tiles_matches_the_small_call():
    """More 64-row tiles than a model has workgroups: the grid-stride loop."""
    import torch
    from afm.mlp import forward_device
    shape, n = (5, 16, 16), 64 * 70 + 9
    X, _, theta = model(shape, n, 4)
    n_pad = (n + 63) // 64 * 64
    Xd, th = planes(X, n_pad), torch.from_numpy(theta).cuda()
    full = forward_device(Xd, th, shape[1:], 0, n).cpu().numpy()
    assert np.isnan(full[:, n:]).all()
    f, E = R.forward_bound(theta[0], X, shape)
    assert (np.abs(full[0, :n].astype(R.LD) - f) <= E).all()
    tail = forward_device(Xd, th, shape[1:], 64 * 66 + 5, 200).cpu().numpy()
    assert tail[0, 64 * 66 + 5:64 * 66 + 205].tobytes() == full[0, 64 * 66 + 5:64 * 66 + 205].tobytes()


# ---- one step on the exact grid ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 16, 16), (29, 128, 32)])
def test_exact_grid_step_bit_for_bit(shape):
    X, y, theta = R.exact_grid(*shape, 256, 11)
    want = R.fit(theta, X, y, 256, 0, shape, lr=1e-3, batch=256, epochs=1)
    got_theta, got_evals, got_snaps = gpu_fit(X, y, 256, 0, shape, theta, 1e-3, 256, 1)
    assert (want["theta"] != theta).mean() > 0.85
    assert got_theta[0].tobytes() == want["theta"].tobytes()
    assert got_evals[0, 0, 0].tobytes() == want["evals"][0, 0].tobytes()
    assert not got_evals[0, 0, 1].any()
    assert got_snaps[0, 0].tobytes() == got_theta[0].tobytes()


# ---- trajectories ------------------------------------------------------------------------------------
# (n_train, n_eval, batch, epochs, lr): batches 256, 256, 88 with eval rows; batch 16 over 1,000
# rows; one short batch (batch > n_train); no eval rows
CASE = {"tail": (600, 100, 256, 3, 1e-3), "small": (1000, 40, 16, 1, 1e-3),
        "short": (150, 30, 256, 4, 1e-3), "noeval": (300, 0, 128, 2, 1e-3)}
TRAJ = [(s, "tail") for s in SHAPES] + [((5, 16, 16), "small"), ((29, 128, 32), "small"),
                                        ((1, 16, 16), "short"), ((64, 128, 64), "short"),
                                        ((5, 16, 16), "noeval"), ((29, 128, 32), "noeval")]


@pytest.mark.parametrize("shape,case", TRAJ)
def test_trajectory_within_the_reference_spread(shape, case):
    n_train, n_eval, batch, epochs, lr = CASE[case]
    X, y, theta = model(shape, n_train + n_eval, 9)
    kw = dict(lr=lr, batch=batch, epochs=epochs)
    a = R.fit(theta[0], X, y, n_train, n_eval, shape, **kw)
    b = R.fit(theta[0], X, y, n_train, n_eval, shape, dtype=R.LD, **kw)
    s = float(max(np.abs(a["snaps"].astype(R.LD) - b["snaps"]).max(),
                  np.abs(a["theta"].astype(R.LD) - b["theta"]).max()))
    assert np.isfinite(s) and s < 1e-9
    tau = 64 * max(s, R.U * float(np.abs(b["theta"]).max()))
    got_theta, got_evals, got_snaps = gpu_fit(X, y, n_train, n_eval, shape, theta, lr, batch, epochs)
    err = float(np.abs(got_theta[0].astype(R.LD) - b["theta"]).max())
    print(shape, case, "steps", len(a["steps"]), "s", s, "tau", tau, "gpu - longdouble", err)
    assert err <= tau
    assert float(np.abs(b["theta"] - theta[0]).max()) > 1e3 * tau          # the fit moved
    assert got_snaps[0, -1].tobytes() == got_theta[0].tobytes()
    snap_err = np.abs(got_snaps[0].astype(R.LD) - b["snaps"]).max()
    assert snap_err <= tau
    # the moments: counts exact, the sums within the rounding of their own summation plus the image
    # of tau (and of the forward bound) on every prediction
    spe = -(-n_train // batch)
    for e in range(epochs):
        delta = np.zeros(n_train, dtype=R.LD)
        for k in range(spe):
            i, j = k * batch, min(k * batch + batch, n_train)
            th = b["steps"][e * spe + k]
            delta[i:j] = R.forward_shift(th, X[i:j], shape, tau) + R.forward_bound(th, X[i:j],
                                                                                   shape)[1]
        tol = R.moments_bound(b["F_train"][e], y[:n_train], delta)
        diff = np.abs(got_evals[0, e, 0].astype(R.LD) - b["evals"][e, 0])
        assert got_evals[0, e, 0, 0] == n_train and (diff <= tol).all(), (e, diff, tol)
        if n_eval:
            Xe, ye = X[n_train:], y[n_train:]
            delta = R.forward_shift(b["snaps"][e], Xe, shape, tau) + \
                R.forward_bound(b["snaps"][e], Xe, shape)[1]
            tol = R.moments_bound(b["F_eval"][e], ye, delta)
            diff = np.abs(got_evals[0, e, 1].astype(R.LD) - b["evals"][e, 1])
            assert got_evals[0, e, 1, 0] == n_eval and (diff <= tol).all(), (e, diff, tol)
        else:
            assert not got_evals[0, e, 1].any()


# ---- invariances, bit for bit ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ensemble():
    shape, n_train, n_eval = (5, 16, 16), 300, 70
    X, y, theta = model(shape, n_train + n_eval, 21, M=3)
    lrs = np.array([1e-3, 3e-3, 5e-4])
    args = dict(batch=64, epochs=2)
    base = gpu_fit(X, y, n_train, n_eval, shape, theta, lrs, **args)
    return shape, n_train, n_eval, X, y, theta, lrs, args, base


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_two_runs_and_steps_per_launch(ensemble):
    shape, n_train, n_eval, X, y, theta, lrs, args, base = ensemble
    assert np.abs(base[0] - theta).max() > 1e-3 and np.isfinite(base[1]).all()
    assert same(base, gpu_fit(X, y, n_train, n_eval, shape, theta, lrs, **args))
    for S in (0, 1, 3, 1 << 20):
        assert same(base, gpu_fit(X, y, n_train, n_eval, shape, theta, lrs, S=S, **args)), S


def test_steps_per_launch_at_the_reference_shape():
    shape, n_train, n_eval = (29, 128, 32), 200, 40
    X, y, theta = model(shape, n_train + n_eval, 22)
    runs = [gpu_fit(X, y, n_train, n_eval, shape, theta, 1e-3, 64, 2, S=S) for S in (0, 1, 3)]
    assert same(runs[0], runs[1]) and same(runs[0], runs[2])


def test_members_together_alone_and_reordered(ensemble):
    shape, n_train, n_eval, X, y, theta, lrs, args, base = ensemble
    for m in range(3):
        alone = gpu_fit(X, y, n_train, n_eval, shape, theta[m], lrs[m], **args)
        assert same([r[m] for r in base], [r[0] for r in alone]), m
    order = [2, 0, 1]
    other = gpu_fit(X, y, n_train, n_eval, shape, theta[order], lrs[order], **args)
    assert same([r[order] for r in base], other)
    assert base[0][0].tobytes() != base[0][1].tobytes()


def test_fit_does_not_depend_on_the_eval_rows(ensemble):
    shape, n_train, n_eval, X, y, theta, lrs, args, base = ensemble
    got = gpu_fit(X, y, n_train, 0, shape, theta, lrs, **args)
    assert got[0].tobytes() == base[0].tobytes() and got[2].tobytes() == base[2].tobytes()
    assert got[1][:, :, 0].tobytes() == np.ascontiguousarray(base[1][:, :, 0]).tobytes()
    assert not got[1][:, :, 1].any() and base[1][:, :, 1, 0].min() == n_eval
    # a larger padding changes nothing either
    wide = gpu_fit(X, y, n_train, n_eval, shape, theta, lrs, n_pad=512, **args)
    assert same(base, wide)


# ---- arguments ---------------------------------------------------------------------------------------
def test_argument_rules_return_without_launching():
    import torch
    from afm import _lib
    from afm.mlp import param_count
    p, h1, h2, M, n_pad = 5, 16, 16, 2, 128
    P = param_count(p, h1, h2)
    f64 = dict(dtype=torch.float64, device="cuda")
    X, y = torch.zeros((p, n_pad), **f64), torch.zeros(n_pad, **f64)
    theta = torch.full((M, P), 0.25, **f64)
    evals, snaps = torch.full((M, 2, 2, 6), -1.0, **f64), torch.full((M, 2, P), -1.0, **f64)
    ctx = _lib.Context.get(0)
    ctx.bind_stream()
    scr = torch.zeros(ctx.call("afm_mlp_scratch_bytes", p, h1, h2, M, 32) // 8 + 2, **f64)
    out = torch.full((M, n_pad), -7.0, **f64)
    good = dict(X=X, y=y, n_pad=n_pad, n_train=100, n_eval=20, p=p, h1=h1, h2=h2, M=M, theta=theta,
                lr=(1e-3, 1e-3), beta1=0.9, beta2=0.999, eps=1e-7, batch=32, epochs=2,
                evals=evals, snaps=snaps, scratch=scr)

    def fit(**kw):
        a = dict(good, **kw)
        a["lr"] = None if a["lr"] is None else (ctypes.c_double * len(a["lr"]))(*a["lr"])
        ctx.call("afm_mlp_fit_f64", *a.values())

    nan, inf = float("nan"), float("inf")
    bad = [dict(p=0), dict(p=65), dict(h1=8), dict(h1=24), dict(h1=144), dict(h2=0), dict(h2=40),
           dict(h1=128, h2=80), dict(p=64, h1=128, h2=80), dict(M=0), dict(M=1025), dict(batch=0),
           dict(batch=4097), dict(epochs=0), dict(epochs=4097), dict(n_train=0), dict(n_eval=-1),
           dict(n_train=100, n_eval=29), dict(n_train=129, n_eval=0), dict(n_pad=100),
           dict(n_pad=0), dict(lr=(1e-3, 0.0)), dict(lr=(-1e-3, 1e-3)), dict(lr=(nan, 1e-3)),
           dict(lr=(1e-3, inf)), dict(lr=None), dict(eps=0.0), dict(eps=nan), dict(eps=inf),
           dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=nan), dict(X=None),
           dict(y=None), dict(theta=None), dict(evals=None), dict(scratch=None),
           dict(X=X.view(-1)[1:]), dict(y=y[1:]), dict(theta=theta.view(-1)[1:]),
           dict(evals=evals.view(-1)[1:]), dict(snaps=snaps.view(-1)[1:]), dict(scratch=scr[1:])]
    for kw in bad:
        with pytest.raises(_lib.AfmError, match="afm_mlp_fit_f64"):
            fit(**kw)
    fwd = dict(X=X, n_pad=n_pad, i0=0, n=100, p=p, h1=h1, h2=h2, M=M, theta=theta, out=out)
    bad = [dict(p=0), dict(p=65), dict(h1=24), dict(h2=144), dict(h1=128, h2=80), dict(M=0),
           dict(M=1025), dict(n_pad=100), dict(i0=-1), dict(n=-1), dict(i0=64, n=65), dict(X=None),
           dict(theta=None), dict(out=None), dict(X=X.view(-1)[1:]), dict(theta=theta.view(-1)[1:]),
           dict(out=out.view(-1)[1:])]
    for kw in bad:
        with pytest.raises(_lib.AfmError, match="afm_mlp_forward_f64"):
            ctx.call("afm_mlp_forward_f64", *dict(fwd, **kw).values())
    torch.cuda.synchronize()
    assert (theta == 0.25).all() and (evals == -1.0).all() and (snaps == -1.0).all()
    assert (out == -7.0).all() and not scr.any()
    # the same calls with every rule met do run
    fit()
    fit(snaps=None)
    ctx.call("afm_mlp_forward_f64", *fwd.values())
    torch.cuda.synchronize()
    assert (theta != 0.25).any() and (evals[:, :, 0, 0] == 100).all()
    assert (evals[:, :, 1, 0] == 20).all() and (out[:, :100] != -7.0).all()
    assert (out[:, 100:] == -7.0).all()
    # and the option is range checked
    for v in (-1, (1 << 20) + 1):
        with pytest.raises(_lib.AfmError):
            ctx.set_option("mlp_steps_per_launch", v)
    assert ctx.get_option("mlp_steps_per_launch") == 0
