"""The recurrent kernels of csrc/lstm.hip against tests/lstm_ref.py: the device sigmoid / tanh
within ACT_ULPS of their longdouble values, the forward values and the BPTT gradient within the
restatement's own spread around its longdouble run (k ascending, k descending, activations nudged
by up to ACT_ULPS ulps), whole trajectories within that spread, the invariances of the fit (runs,
rows per workgroup, ensemble composition, eval rows) bit for bit, and the argument rules."""
import ctypes

import numpy as np
import pytest

import lstm_ref as R

pytestmark = pytest.mark.gpu

FWD_SHAPES = [(1, 1, 4, 4), (3, 2, 4, 8), (8, 1, 16, 16), (29, 1, 32, 16), (4, 3, 100, 100),
              (98, 1, 16, 16), (2, 64, 128, 128)]
GRAD_SHAPES = FWD_SHAPES[:-1]


def planes(X, n_pad, y=None, poison=True):
    """device X [T][d][n_pad] (and y [n_pad]) from host X [n][T][d], with NaN / inf in every cell
    past the rows of X."""
    import torch
    n, T, d = X.shape
    Xp = np.full((T, d, n_pad), np.nan if poison else 0.0)
    Xp[:, :, n:][:, :, ::2] = np.inf if poison else 0.0
    Xp[:, :, :n] = X.transpose(1, 2, 0)
    out = [torch.from_numpy(Xp).cuda()]
    if y is not None:
        yp = np.full(n_pad, np.nan if poison else 0.0)
        yp[:n] = y
        out.append(torch.from_numpy(yp).cuda())
    return out if y is not None else out[0]


def model(shape, n, seed, M=1):
    from afm.lstm import lstm_init
    T, d, h1, h2 = shape
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, T, d))
    y = 0.1 * rng.standard_normal(n)
    theta = np.stack([lstm_init(d, (h1, h2), seed + m) for m in range(M)])
    theta += 0.05 * rng.standard_normal(theta.shape)
    return X, y, theta


def spread(fn):
    """(longdouble value, s): fn(**kw) in longdouble, and the largest distance from it of the fp64
    restatements (k ascending, k descending, activations nudged by ACT_ULPS ulps)."""
    ld = fn(dtype=R.LD)
    s = max(float(np.abs(fn(**kw).astype(R.LD) - ld).max()) for kw in R.variants())
    return ld, s


def gpu_fit(X, y, n_train, n_eval, shape, theta0, lrs, batch, epochs, rows=None, n_pad=None,
            **adam):
    """afm.lstm.fit_device on poisoned planes -> host (theta [M][P], evals, snaps)."""
    import torch
    from afm import _lib
    from afm.lstm import LSTMParams, fit_device
    theta0 = np.atleast_2d(theta0)
    M = len(theta0)
    n_pad = n_pad or (len(y) + 63) // 64 * 64
    Xd, yd = planes(X[:n_train + n_eval], n_pad, y[:n_train + n_eval])
    prm = LSTMParams(hidden=shape[2:], lr=tuple(np.broadcast_to(lrs, M).tolist()), epochs=epochs,
                     batch_size=batch, seeds=tuple(range(M)), **adam)
    if rows is None:
        res = fit_device(Xd, yd, n_train, n_eval, prm, theta0=theta0)
    else:
        with _lib.options(lstm_rows_per_wg=rows):
            res = fit_device(Xd, yd, n_train, n_eval, prm, theta0=theta0)
    torch.cuda.synchronize()
    return tuple(res[k].cpu().numpy() for k in ("theta", "evals", "snaps"))


# ---- activations -----------------------------------------------------------------------------------
def test_device_sigmoid_and_tanh_within_act_ulps():
    import torch
    from afm import _lib
    rng = np.random.default_rng(1)
    x = np.concatenate([np.linspace(-40.0, 40.0, 60001), rng.uniform(-40, 40, 40000),
                        rng.uniform(-2, 2, 20000)])
    big = np.array([0.0, 745.0, -745.0, 1e3, -1e3])
    xd = torch.from_numpy(np.concatenate([x, big])).cuda()
    out = torch.full_like(xd, -7.0)
    xl = x.astype(R.LD)
    want = {0: R.LD(1) / (R.LD(1) + np.exp(-xl)), 1: np.tanh(xl)}
    limits = {0: [0.5, 1.0, 0.0, 1.0, 0.0], 1: [0.0, 1.0, -1.0, 1.0, -1.0]}
    for kind in (0, 1):
        _lib.run("afm_lstm_act_f64", kind, xd, len(xd), out)
        got = out.cpu().numpy()
        ulps = np.abs(got[:len(x)].astype(R.LD) - want[kind]) / np.spacing(np.abs(got[:len(x)]))
        print("kind", kind, "max error in ulps", float(ulps.max()))
        assert float(ulps.max()) <= R.ACT_ULPS
        assert got[len(x):].tolist() == limits[kind]
    _lib.run("afm_lstm_act_f64", 0, xd, 0, out)                  # n = 0: nothing
    assert out.cpu().numpy().tobytes() == got.tobytes()


# ---- forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_forward_within_the_spread_and_slices_bitwise(shape):
    import torch
    from afm.lstm import forward_device
    n, n_pad, M = 200, 256, 2
    X, _, theta = model(shape, n, 3, M)
    Xd = planes(X, n_pad)
    th = torch.from_numpy(theta).cuda()
    out = torch.full((M, n_pad), -7.0, dtype=torch.float64, device="cuda")
    forward_device(Xd, th, shape[2:], 0, n, out=out)
    full = out.cpu().numpy()
    assert (full[:, n:] == -7.0).all() and np.isfinite(full[:, :n]).all()
    for m in range(M):
        f, s = spread(lambda **kw: R.forward(theta[m], X, shape, **kw))
        tol = 64 * max(s, R.U * float(np.abs(f).max()))
        err = float(np.abs(full[m, :n].astype(R.LD) - f).max())
        print(shape, m, "s", s, "tol", tol, "gpu - longdouble", err)
        assert err <= tol
    # a window that is no multiple of the tile, at an offset that is none either
    for i0, k in ((37, 101), (64, 64), (199, 1), (3, 13)):
        out = torch.full((M, n_pad), -7.0, dtype=torch.float64, device="cuda")
        forward_device(Xd, th, shape[2:], i0, k, out=out)
        part = out.cpu().numpy()
        assert part[:, i0:i0 + k].tobytes() == full[:, i0:i0 + k].tobytes()
        assert (part[:, :i0] == -7.0).all() and (part[:, i0 + k:] == -7.0).all()
    forward_device(Xd, th, shape[2:], 5, 0, out=out)          # n = 0: nothing
    assert out.cpu().numpy().tobytes() == part.tobytes()


def test_forward_over_more_row_groups_than_workgroups():
    """More row groups than a model has workgroups: the grid-stride loop, at every group size."""
    import torch
    from afm import _lib
    from afm.lstm import forward_device
    shape, n = (3, 2, 4, 8), 64 * 70 + 9
    X, _, theta = model(shape, n, 4)
    n_pad = (n + 63) // 64 * 64
    Xd, th = planes(X, n_pad), torch.from_numpy(theta).cuda()
    full = forward_device(Xd, th, shape[2:], 0, n).cpu().numpy()
    assert np.isnan(full[:, n:]).all()
    f, s = spread(lambda **kw: R.forward(theta[0], X, shape, **kw))
    assert np.abs(full[0, :n].astype(R.LD) - f).max() <= 64 * max(s, R.U * float(np.abs(f).max()))
    lo = 64 * 66 + 5
    tail = forward_device(Xd, th, shape[2:], lo, 200).cpu().numpy()
    assert tail[0, lo:lo + 200].tobytes() == full[0, lo:lo + 200].tobytes()
    for rows in (16, 32, 48, 64):
        with _lib.options(lstm_rows_per_wg=rows):
            other = forward_device(Xd, th, shape[2:], 0, n).cpu().numpy()
        assert other[:, :n].tobytes() == full[:, :n].tobytes(), rows


# ---- the gradient of one batch -----------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 16, 100, 256])
@pytest.mark.parametrize("shape", GRAD_SHAPES)
def test_gradient_within_the_spread(shape, nb):
    import torch
    from afm.lstm import grad_device
    T, d, h1, h2 = shape
    i0, n_pad = 21, 320
    X, y, theta = model(shape, i0 + nb + 5, 7)
    Xd, yd = planes(X, n_pad, y)
    grad, F = grad_device(Xd, yd, torch.from_numpy(theta).cuda(), shape[2:], i0, nb)
    torch.cuda.synchronize()
    grad, F = grad.cpu().numpy()[0], F.cpu().numpy()[0]
    Xb, yb = X[i0:i0 + nb], y[i0:i0 + nb]
    g, f = R.gradient(theta[0], Xb, yb, shape, dtype=R.LD)
    runs = [R.gradient(theta[0], Xb, yb, shape, **kw) for kw in R.variants()]
    s = max(float(np.abs(a[0].astype(R.LD) - g).max()) for a in runs)
    sf = max(float(np.abs(a[1].astype(R.LD) - f).max()) for a in runs)
    tol = 64 * max(s, R.U * float(np.abs(g).max()))
    err = np.abs(grad.astype(R.LD) - g)
    print(shape, nb, "s", s, "tol", tol, "gpu - longdouble", float(err.max()))
    assert np.isfinite(grad).all() and (err <= tol).all()
    # no block passes by being zero -- but at T = 1 the recurrent rows of K1 meet only h_0 = 0: their
    # gradient is exactly zero, in the restatement and on the device
    for name, sl in R.blocks(d, h1, h2).items():
        if T == 1 and name == "K1h":
            assert not g[sl].any() and not grad[sl].any()
        else:
            assert np.abs(g[sl]).max() > 0, name
    assert np.isnan(F[:i0]).all() and np.isnan(F[i0 + nb:]).all()
    assert np.abs(F[i0:i0 + nb].astype(R.LD) - f).max() <= 64 * max(sf, R.U * float(np.abs(f).max()))


# ---- trajectories ------------------------------------------------------------------------------------
# shape -> (n_train, n_eval, batch, epochs): batches 256, 256, 88 with eval rows; T = 29 with eval
# rows; one short batch (batch > n_train) at the reference's widths, no eval rows; T = 98
TRAJ = {(8, 1, 16, 16): (600, 100, 256, 3), (29, 1, 32, 16): (300, 50, 128, 2),
        (6, 3, 100, 100): (150, 0, 256, 2), (98, 1, 16, 16): (128, 0, 64, 2)}


def shift_under_perturbation(theta, X, shape, tau, F):
    """The largest change of every row's longdouble prediction when every entry of theta moves by
    +tau or -tau (a seeded sign pattern and its mirror image)."""
    sign = np.random.default_rng(5).choice([-1.0, 1.0], size=len(theta)).astype(R.LD)
    out = np.zeros(len(X), dtype=R.LD)
    for sg in (sign, -sign):
        out = np.maximum(out, np.abs(R.forward(theta + R.LD(tau) * sg, X, shape, dtype=R.LD) - F))
    return out


@pytest.mark.parametrize("shape", list(TRAJ))
def test_trajectory_within_the_reference_spread(shape):
    """theta and every snapshot within tau = 64 max(s, u max|theta|) of the longdouble fit, s the
    restatement's own spread.  The moment sums are bounded by mlp_ref.moments_bound with, per
    prediction, delta = 64 x (the largest change of that prediction over the restatements + its
    change under a +-tau perturbation of theta in longdouble): the factor of the trajectory rule
    applied to the restatement's measured shift of the prediction itself."""
    n_train, n_eval, batch, epochs = TRAJ[shape]
    lr = 1e-3
    X, y, theta = model(shape, n_train + n_eval, 9)
    kw = dict(lr=lr, batch=batch, epochs=epochs)
    b = R.fit(theta[0], X, y, n_train, n_eval, shape, dtype=R.LD, **kw)
    runs = [R.fit(theta[0], X, y, n_train, n_eval, shape, **kw, **v) for v in R.variants()]
    s = float(max(max(np.abs(a["snaps"].astype(R.LD) - b["snaps"]).max(),
                      np.abs(a["theta"].astype(R.LD) - b["theta"]).max()) for a in runs))
    assert np.isfinite(s) and s < 1e-9
    tau = 64 * max(s, R.U * float(np.abs(b["theta"]).max()))
    got_theta, got_evals, got_snaps = gpu_fit(X, y, n_train, n_eval, shape, theta, lr, batch, epochs)
    err = float(np.abs(got_theta[0].astype(R.LD) - b["theta"]).max())
    moved = float(np.abs(b["theta"] - theta[0]).max())
    print(shape, "steps", len(b["steps"]), "s", s, "tau", tau, "gpu - longdouble", err,
          "= %.2f s" % (err / s), "moved", moved)
    assert err <= tau
    assert moved > 1e3 * tau                                               # the fit moved
    assert got_snaps[0, -1].tobytes() == got_theta[0].tobytes()
    assert np.abs(got_snaps[0].astype(R.LD) - b["snaps"]).max() <= tau
    spe = -(-n_train // batch)
    for e in range(epochs):
        delta = np.zeros(n_train, dtype=R.LD)
        for k in range(spe):
            i, j = k * batch, min(k * batch + batch, n_train)
            delta[i:j] = shift_under_perturbation(b["steps"][e * spe + k], X[i:j], shape, tau,
                                                  b["F_train"][e, i:j])
        delta = delta + np.max([np.abs(a["F_train"][e].astype(R.LD) - b["F_train"][e])
                                for a in runs], axis=0)
        tol = R.moments_bound(b["F_train"][e], y[:n_train], 64 * delta)
        diff = np.abs(got_evals[0, e, 0].astype(R.LD) - b["evals"][e, 0])
        assert got_evals[0, e, 0, 0] == n_train and (diff <= tol).all(), (e, diff, tol)
        if n_eval:
            Xe, ye = X[n_train:], y[n_train:]
            delta = shift_under_perturbation(b["snaps"][e], Xe, shape, tau, b["F_eval"][e])
            delta = delta + np.max([np.abs(a["F_eval"][e].astype(R.LD) - b["F_eval"][e])
                                    for a in runs], axis=0)
            tol = R.moments_bound(b["F_eval"][e], ye, 64 * delta)
            diff = np.abs(got_evals[0, e, 1].astype(R.LD) - b["evals"][e, 1])
            assert got_evals[0, e, 1, 0] == n_eval and (diff <= tol).all(), (e, diff, tol)
        else:
            assert not got_evals[0, e, 1].any()


# ---- invariances, bit for bit ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ensemble():
    shape, n_train, n_eval = (5, 2, 8, 8), 300, 70
    X, y, theta = model(shape, n_train + n_eval, 21, M=3)
    lrs = np.array([1e-3, 3e-3, 5e-4])
    args = dict(batch=64, epochs=2)
    base = gpu_fit(X, y, n_train, n_eval, shape, theta, lrs, **args)
    return shape, n_train, n_eval, X, y, theta, lrs, args, base


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_two_runs_and_rows_per_workgroup(ensemble):
    shape, n_train, n_eval, X, y, theta, lrs, args, base = ensemble
    assert np.abs(base[0] - theta).max() > 1e-3 and np.isfinite(base[1]).all()
    assert (base[1][:, :, 0, 0] == n_train).all() and (base[1][:, :, 1, 0] == n_eval).all()
    assert same(base, gpu_fit(X, y, n_train, n_eval, shape, theta, lrs, **args))
    for rows in (16, 32, 64):
        assert same(base, gpu_fit(X, y, n_train, n_eval, shape, theta, lrs, rows=rows, **args)), rows


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


def tile_moments(F, y):
    """The six moments as the kernels add them: every 16-row tile row after row from 0.0, the tiles
    one after the other onto the running sums."""
    mom = np.zeros(6)
    for r0 in range(0, len(F), 16):
        p = np.zeros(6)
        for f, v in zip(F[r0:r0 + 16], y[r0:r0 + 16]):
            p = p + np.array([1.0, f, v, f * f, v * v, f * v])
        mom = mom + p
    return mom


def test_gradient_call_equals_the_first_step_of_the_fit(ensemble):
    """afm_lstm_grad_f64 on the first batch: the Adam recurrence of afm_mlp.h applied to it on the
    host gives the fit's parameters after its first step bit for bit, and its predictions give the
    fit's slot-0 moments bit for bit (the same F bytes)."""
    import torch
    from afm.lstm import grad_device
    shape, n_train, n_eval, X, y, theta, lrs, args, base = ensemble
    nb = args["batch"]
    one = gpu_fit(X, y, nb, 0, shape, theta, lrs, batch=nb, epochs=1)
    Xd, yd = planes(X[:nb], 64, y[:nb])
    grad, F = grad_device(Xd, yd, torch.from_numpy(theta).cuda(), shape[2:], 0, nb)
    grad, F = grad.cpu().numpy(), F.cpu().numpy()
    for m in range(3):
        st = R.adam_state(theta.shape[1])
        want = R.adam_step(theta[m], grad[m], st, lrs[m], 0.9, 0.999, 1e-7)
        assert one[0][m].tobytes() == want.tobytes(), m
        assert one[1][m, 0, 0].tobytes() == tile_moments(F[m, :nb], y[:nb]).tobytes(), m
    # and the first step of the longer fit made the same predictions: the same gradient call on
    # poisoned planes of the whole design
    Xd, yd = planes(X, 384, y)
    grad2, F2 = grad_device(Xd, yd, torch.from_numpy(theta).cuda(), shape[2:], 0, nb)
    assert grad2.cpu().numpy().tobytes() == grad.tobytes()
    assert F2.cpu().numpy()[:, :nb].tobytes() == F[:, :nb].tobytes()


# ---- arguments ---------------------------------------------------------------------------------------
def test_argument_rules_return_without_launching():
    import torch
    from afm import _lib
    from afm.lstm import param_count
    T, d, h1, h2, M, n_pad = 5, 2, 4, 8, 2, 128
    P = param_count(d, h1, h2)
    f64 = dict(dtype=torch.float64, device="cuda")
    X, y = torch.zeros((T, d, n_pad), **f64), torch.zeros(n_pad, **f64)
    theta = torch.full((M, P), 0.25, **f64)
    evals, snaps = torch.full((M, 2, 2, 6), -1.0, **f64), torch.full((M, 2, P), -1.0, **f64)
    grad = torch.full((M, P), -3.0, **f64)
    ctx = _lib.Context.get(0)
    ctx.bind_stream()
    scr = torch.zeros(ctx.call("afm_lstm_scratch_bytes", T, d, h1, h2, M, 32) // 8 + 2, **f64)
    out = torch.full((M, n_pad), -7.0, **f64)
    good = dict(X=X, y=y, n_pad=n_pad, n_train=100, n_eval=20, T=T, d=d, h1=h1, h2=h2, M=M,
                theta=theta, lr=(1e-3, 1e-3), beta1=0.9, beta2=0.999, eps=1e-7, batch=32, epochs=2,
                evals=evals, snaps=snaps, scratch=scr)

    def fit(**kw):
        a = dict(good, **kw)
        a["lr"] = None if a["lr"] is None else (ctypes.c_double * len(a["lr"]))(*a["lr"])
        ctx.call("afm_lstm_fit_f64", *a.values())

    nan, inf = float("nan"), float("inf")
    shapes = [dict(T=0), dict(T=257), dict(d=0), dict(d=65), dict(h1=0), dict(h1=6), dict(h1=132),
              dict(h2=2), dict(h2=10), dict(h2=132), dict(M=0), dict(M=65), dict(n_pad=100),
              dict(n_pad=0)]
    bad = shapes + [dict(batch=0), dict(batch=1025), dict(epochs=0), dict(epochs=4097),
                    dict(n_train=0), dict(n_eval=-1), dict(n_train=100, n_eval=29),
                    dict(n_train=129, n_eval=0), dict(lr=(1e-3, 0.0)), dict(lr=(-1e-3, 1e-3)),
                    dict(lr=(nan, 1e-3)), dict(lr=(1e-3, inf)), dict(lr=None), dict(eps=0.0),
                    dict(eps=nan), dict(eps=inf), dict(beta1=1.0), dict(beta1=-0.1),
                    dict(beta2=1.0), dict(beta2=nan), dict(X=None), dict(y=None), dict(theta=None),
                    dict(evals=None), dict(scratch=None), dict(X=X.view(-1)[1:]), dict(y=y[1:]),
                    dict(theta=theta.view(-1)[1:]), dict(evals=evals.view(-1)[1:]),
                    dict(snaps=snaps.view(-1)[1:]), dict(scratch=scr[1:])]
    for kw in bad:
        with pytest.raises(_lib.AfmError, match="afm_lstm_fit_f64"):
            fit(**kw)
    gr = dict(X=X, y=y, n_pad=n_pad, i0=3, nb=32, T=T, d=d, h1=h1, h2=h2, M=M, theta=theta,
              grad=grad, F=out, scratch=scr)
    bad = shapes + [dict(nb=0), dict(nb=1025), dict(i0=-1), dict(i0=100, nb=29), dict(X=None),
                    dict(y=None), dict(theta=None), dict(grad=None), dict(scratch=None),
                    dict(grad=grad.view(-1)[1:]), dict(F=out.view(-1)[1:]), dict(scratch=scr[1:])]
    for kw in bad:
        with pytest.raises(_lib.AfmError, match="afm_lstm_grad_f64"):
            ctx.call("afm_lstm_grad_f64", *dict(gr, **kw).values())
    fwd = dict(X=X, n_pad=n_pad, i0=0, n=100, T=T, d=d, h1=h1, h2=h2, M=M, theta=theta, out=out)
    bad = shapes + [dict(i0=-1), dict(n=-1), dict(i0=64, n=65), dict(X=None), dict(theta=None),
                    dict(out=None), dict(X=X.view(-1)[1:]), dict(theta=theta.view(-1)[1:]),
                    dict(out=out.view(-1)[1:])]
    for kw in bad:
        with pytest.raises(_lib.AfmError, match="afm_lstm_forward_f64"):
            ctx.call("afm_lstm_forward_f64", *dict(fwd, **kw).values())
    for kw in (dict(kind=2), dict(kind=-1), dict(n=-1), dict(x=None), dict(out=None)):
        with pytest.raises(_lib.AfmError, match="afm_lstm_act_f64"):
            ctx.call("afm_lstm_act_f64", *dict(dict(kind=0, x=y, n=64, out=out), **kw).values())
    torch.cuda.synchronize()
    assert (theta == 0.25).all() and (evals == -1.0).all() and (snaps == -1.0).all()
    assert (out == -7.0).all() and (grad == -3.0).all() and not scr.any()
    # the same calls with every rule met do run
    ctx.call("afm_lstm_grad_f64", *gr.values())
    torch.cuda.synchronize()
    assert (grad != -3.0).all() and (out[:, 3:35] != -7.0).all() and (out[:, 35:] == -7.0).all()
    out.fill_(-7.0)
    fit()
    fit(snaps=None)
    ctx.call("afm_lstm_forward_f64", *fwd.values())
    torch.cuda.synchronize()
    assert (theta != 0.25).any() and (evals[:, :, 0, 0] == 100).all()
    assert (evals[:, :, 1, 0] == 20).all() and (out[:, :100] != -7.0).all()
    assert (out[:, 100:] == -7.0).all()
    # and the option is range checked
    for v in (-16, 8, 24, 80):
        with pytest.raises(_lib.AfmError):
            ctx.set_option("lstm_rows_per_wg", v)
    assert ctx.get_option("lstm_rows_per_wg") == 0
