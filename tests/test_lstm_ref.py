"""tests/lstm_ref.py, the numpy restatement of include/afm_lstm.h, against independent statements
(no GPU needed): torch.nn.LSTM with autograd on the CPU, central differences of the longdouble
loss, and the properties of afm.lstm.lstm_init."""
import numpy as np
import pytest

import lstm_ref as R


def case(shape, n, seed):
    from afm.lstm import lstm_init
    T, d, h1, h2 = shape
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, T, d))
    y = 0.1 * rng.standard_normal(n)
    theta = lstm_init(d, (h1, h2), seed)
    theta = theta + 0.05 * rng.standard_normal(theta.shape)
    return X, y, theta


@pytest.mark.parametrize("shape", [(5, 2, 4, 8), (8, 1, 16, 16)])
def test_predictions_and_gradient_agree_with_torch_autograd(shape):
    import torch
    T, d, h1, h2 = shape
    n = 9
    X, y, theta = case(shape, n, 3)
    g64, F64 = R.gradient(theta, X, y, shape)
    gld, Fld = R.gradient(theta, X, y, shape, dtype=R.LD)
    K1, b1, K2, b2, w, b3 = R.unpack(theta, d, h1, h2)
    l1 = torch.nn.LSTM(d, h1, batch_first=True).double()
    l2 = torch.nn.LSTM(h1, h2, batch_first=True).double()
    head = torch.nn.Linear(h2, 1).double()
    with torch.no_grad():                       # torch's gate order is i, f, g, o too
        for lay, K, b, din in ((l1, K1, b1, d), (l2, K2, b2, h1)):
            lay.weight_ih_l0.copy_(torch.from_numpy(np.ascontiguousarray(K[:din].T)))
            lay.weight_hh_l0.copy_(torch.from_numpy(np.ascontiguousarray(K[din:].T)))
            lay.bias_ih_l0.copy_(torch.from_numpy(b))
            lay.bias_hh_l0.zero_()
        head.weight.copy_(torch.from_numpy(w[None, :]))
        head.bias.copy_(torch.from_numpy(b3))
    o1, _ = l1(torch.from_numpy(X))
    o2, _ = l2(o1)
    F = head(o2[:, -1, :])[:, 0]
    loss = ((F - torch.from_numpy(y)) ** 2).mean()
    loss.backward()
    gt = np.concatenate([l1.weight_ih_l0.grad.numpy().T.ravel(),
                         l1.weight_hh_l0.grad.numpy().T.ravel(), l1.bias_ih_l0.grad.numpy(),
                         l2.weight_ih_l0.grad.numpy().T.ravel(),
                         l2.weight_hh_l0.grad.numpy().T.ravel(), l2.bias_ih_l0.grad.numpy(),
                         head.weight.grad.numpy().ravel(), head.bias.grad.numpy()])
    sF = float(np.abs(F64.astype(R.LD) - Fld).max())
    sg = float(np.abs(g64.astype(R.LD) - gld).max())
    tolF = 64 * max(sF, R.U * float(np.abs(Fld).max()))
    tolg = 64 * max(sg, R.U * float(np.abs(gld).max()))
    eF = float(np.abs(F.detach().numpy() - F64).max())
    eg = float(np.abs(gt - g64).max())
    print(shape, "F", eF, "tol", tolF, "grad", eg, "tol", tolg)
    assert eF <= tolF and eg <= tolg
    assert np.abs(g64).max() > 1e-3


def test_longdouble_gradient_against_central_differences():
    shape, n, h = (5, 2, 4, 4), 7, 1e-7
    T, d, h1, h2 = shape
    X, y, theta = case(shape, n, 5)
    g, _ = R.gradient(theta, X, y, shape, dtype=R.LD)

    def loss(th):
        F = R.forward(th, X, shape, dtype=R.LD)
        r = F - y.astype(R.LD)
        return (r * r).sum() / R.LD(n)
    th = theta.astype(R.LD)
    fd = np.zeros(len(th), R.LD)
    for q in range(len(th)):
        e = np.zeros(len(th), R.LD)
        e[q] = R.LD(h)
        fd[q] = (loss(th + e) - loss(th - e)) / (2 * R.LD(h))
    err = float(np.abs(fd - g).max())
    print("central differences", err, "max |g|", float(np.abs(g).max()))
    assert err <= 1e-10 and np.abs(g).max() > 1e-2
    # every parameter block has a gradient
    for name, sl in R.blocks(d, h1, h2).items():
        assert np.abs(g[sl]).max() > 0, name


def test_reversed_and_nudged_restatements_stay_close_and_differ():
    shape = (5, 2, 4, 8)
    X, y, theta = case(shape, 20, 6)
    gld, _ = R.gradient(theta, X, y, shape, dtype=R.LD)
    runs = [R.gradient(theta, X, y, shape, **kw)[0] for kw in R.variants()]
    for g in runs:
        assert np.abs(g.astype(R.LD) - gld).max() < 1e-13
    assert runs[0].tobytes() != runs[1].tobytes() and runs[0].tobytes() != runs[2].tobytes()
    a = R.Acts(np.float64, ulps=3, seed=2)
    v = np.linspace(0.1, 0.9, 1000)
    moved = np.rint((a.nudge(v) - v) / np.spacing(v)).astype(int)
    assert moved.min() == -3 and moved.max() == 3 and set(np.unique(moved)) == set(range(-3, 4))


def test_fit_restatement_counts_steps_and_moments():
    shape = (3, 2, 4, 4)
    X, y, theta = case(shape, 50, 7)
    r = R.fit(theta, X, y, 40, 10, shape, lr=1e-3, batch=16, epochs=2)
    assert len(r["steps"]) == 6 and r["snaps"].shape == (2, len(theta))
    assert r["evals"][:, 0, 0].tolist() == [40, 40] and r["evals"][:, 1, 0].tolist() == [10, 10]
    assert r["snaps"][-1].tobytes() == r["theta"].tobytes()
    # slot 0 holds the predictions each step made before its update
    F0 = R.forward(theta, X[:16], shape)
    assert r["F_train"][0, :16].tobytes() == F0.tobytes()
    none = R.fit(theta, X, y, 40, 0, shape, lr=1e-3, batch=16, epochs=1)
    assert not none["evals"][0, 1].any() and none["snaps"][0].tobytes() == r["snaps"][0].tobytes()


def test_lstm_init_is_keras_default():
    from afm.lstm import lstm_init, param_count
    assert param_count(1, 100, 100) == 121301 == R.param_count(1, 100, 100)
    assert param_count(29, 128, 64) == R.param_count(29, 128, 64)
    d, h1, h2 = 1, 100, 100
    th = lstm_init(d, (h1, h2), 2023)
    assert th.shape == (121301,) and th.tobytes() == lstm_init(d, (h1, h2), 2023).tobytes()
    assert th.tobytes() != lstm_init(d, (h1, h2), 2024).tobytes()
    K1, b1, K2, b2, w, b3 = R.unpack(th, d, h1, h2)
    for K, b, din, H in ((K1, b1, d, h1), (K2, b2, h1, h2)):
        rec = K[din:]
        assert np.abs(rec @ rec.T - np.eye(H)).max() <= 1e-12          # orthonormal rows
        lim = np.sqrt(6.0 / (din + 4 * H))
        assert np.abs(K[:din]).max() <= lim and np.abs(K[:din]).max() > 0.5 * lim
        assert (b[H:2 * H] == 1.0).all() and not b[:H].any() and not b[2 * H:].any()
    lim = np.sqrt(6.0 / (h2 + 1))
    assert np.abs(w).max() <= lim and w.std() > 0.3 * lim and b3[0] == 0.0
    small = lstm_init(3, (4, 8), 1)
    assert small.shape == (R.param_count(3, 4, 8),)
