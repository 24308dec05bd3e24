"""tests/mlp_ref.py against itself and against torch autograd (no GPU): the fp64 forward inside the
derived bound, the running learning rate, the initialiser, the gradient, the exact grid on which
two summation orders agree to the last bit, and the spread of a trajectory between fp64 and
longdouble -- the quantities the GPU tests' tolerances are built from."""
import numpy as np
import pytest

import mlp_ref as R

SHAPES = [(1, 16, 16), (5, 16, 16), (29, 128, 32), (64, 128, 64)]


def model(shape, n, seed):
    from afm.mlp import glorot_init
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, shape[0]))
    theta = glorot_init(shape[0], shape[1:], seed)
    theta += 0.05 * rng.standard_normal(len(theta))           # biases off zero
    y = 0.1 * rng.standard_normal(n)
    return X, y, theta


@pytest.mark.parametrize("shape", SHAPES)
def test_fp64_forward_lies_within_the_bound(shape):
    X, _, theta = model(shape, 96, 3)
    f, E = R.forward_bound(theta, X, shape)
    assert (E > 0).all() and E.max() < 1e-10
    for rev in (False, True):
        got = R.forward(theta, X, shape, np.float64, rev)[4]
        err = np.abs(got.astype(R.LD) - f)
        print(shape, rev, float((err / E).max()))
        assert (err <= E).all()
    # a dropped term is far outside it
    th = theta.copy()
    th[0] = 0.0
    off = np.abs(R.forward(th, X, shape)[4].astype(R.LD) - f)
    assert (off > E).any()


def test_running_learning_rate_against_the_closed_form():
    """The running powers carry one rounding a step: after t steps b2p is within t u of beta2^t
    (relative), which 1 - b2p magnifies by b2p / (1 - b2p) and the root halves; likewise b1p without
    the root; four more roundings in the quotient itself.  The observed error is tens of u at the
    most (the first steps, where 1 - beta2^t is small)."""
    st = R.adam_state(1)
    worst = 0.0
    for t in range(1, 1001):
        got = R.lr_t(st, 1e-4, 0.9, 0.999)
        p1, p2 = pow(R.LD(0.9), t), pow(R.LD(0.999), t)
        want = 1e-4 * np.sqrt(1.0 - p2) / (1.0 - p1)
        bound = R.U * (0.5 * t * p2 / (1.0 - p2) + t * p1 / (1.0 - p1) + 4)
        rel = float(abs(got - want) / want)
        assert rel <= bound, t
        worst = max(worst, rel)
    print("lr_t relative error", worst / R.U, "u")
    assert worst <= 1024 * R.U


def test_glorot_init_limits_and_determinism():
    from afm.mlp import glorot_init, param_count
    for p, h1, h2 in SHAPES:
        t = glorot_init(p, (h1, h2), 7)
        assert t.shape == (param_count(p, h1, h2),) == (R.param_count(p, h1, h2),)
        W1, b1, W2, b2, w3, b3 = R.unpack(t, p, h1, h2)
        for W, fi, fo in ((W1, p, h1), (W2, h1, h2), (w3, h2, 1)):
            lim = np.sqrt(6.0 / (fi + fo))
            assert np.abs(W).max() < lim and np.abs(W).max() > 0.5 * lim
        assert not b1.any() and not b2.any() and not b3.any()
        assert np.array_equal(t, glorot_init(p, (h1, h2), 7))
        assert not np.array_equal(t, glorot_init(p, (h1, h2), 8))
    assert param_count(29, 128, 32) == 8001


@pytest.mark.parametrize("shape", SHAPES[1:3])
def test_gradient_against_autograd(shape):
    import torch
    p, h1, h2 = shape
    X, y, theta = model(shape, 40, 5)
    g64, _ = R.gradient(theta, X, y, shape)
    gld, _ = R.gradient(theta, X, y, shape, R.LD)
    own = float(np.abs(g64.astype(R.LD) - gld).max())
    t = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    o, parts = 0, []
    for s in ((p, h1), (h1,), (h1, h2), (h2,), (h2,), (1,)):
        k = int(np.prod(s))
        parts.append(t[o:o + k].reshape(s))
        o += k
    W1, b1, W2, b2, w3, b3 = parts
    Xt, yt = torch.tensor(X), torch.tensor(y)
    f = torch.relu(torch.relu(Xt @ W1 + b1) @ W2 + b2) @ w3 + b3
    ((f - yt) ** 2).mean().backward()
    diff = float(np.abs(t.grad.numpy() - g64).max())
    print(shape, "autograd diff", diff, "own fp64-longdouble diff", own)
    assert own > 0 and diff <= 64 * own


@pytest.mark.parametrize("shape", [(5, 16, 16), (29, 128, 32)])
def test_exact_grid_two_orders_same_bits(shape):
    X, y, theta = R.exact_grid(*shape, 256, 11)
    kw = dict(lr=1e-3, batch=256, epochs=1)
    a = R.fit(theta, X, y, 256, 0, shape, **kw)
    b = R.fit(theta, X, y, 256, 0, shape, rev=True, **kw)
    c = R.fit(theta, X, y, 256, 0, shape, dtype=R.LD, **kw)
    assert a["theta"].tobytes() == b["theta"].tobytes()
    assert a["evals"].tobytes() == b["evals"].tobytes()
    assert np.array_equal(a["evals"].astype(R.LD), c["evals"])      # the moments are exact
    changed = (a["theta"] != theta).mean()
    print(shape, "changed", changed)
    assert changed > 0.85


CASES = [((5, 16, 16), 600, 100, 256, 3, 1e-3), ((29, 128, 32), 300, 50, 64, 2, 1e-2),
         ((5, 16, 16), 1000, 0, 16, 2, 1e-3)]


@pytest.mark.parametrize("shape,n_train,n_eval,batch,epochs,lr", CASES)
def test_trajectory_spread_is_rounding_sized(shape, n_train, n_eval, batch, epochs, lr):
    X, y, theta = model(shape, n_train + n_eval, 9)
    kw = dict(lr=lr, batch=batch, epochs=epochs)
    a = R.fit(theta, X, y, n_train, n_eval, shape, **kw)
    b = R.fit(theta, X, y, n_train, n_eval, shape, dtype=R.LD, **kw)
    c = R.fit(theta, X, y, n_train, n_eval, shape, rev=True, **kw)
    s = float(np.abs(a["theta"].astype(R.LD) - b["theta"]).max())
    s_rev = float(np.abs(c["theta"].astype(R.LD) - b["theta"]).max())
    moved = float(np.abs(a["theta"] - theta).max())
    print(shape, "steps", len(a["steps"]), "s", s, "alternate order", s_rev, "moved", moved)
    assert np.isfinite(s) and s < 1e-9 and moved > 1e-3
    assert a["evals"].shape == (epochs, 2, 6) and a["evals"][0, 0, 0] == n_train
    assert a["evals"][0, 1, 0] == n_eval
    assert a["snaps"][-1].tobytes() == a["theta"].tobytes()
