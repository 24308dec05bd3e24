"""The numpy restatement of include/afm_lstm.h: the network LSTM(H1) -> LSTM(H2) -> Dense(1), its
gradient by back-propagation through time, one Adam step (tests/mlp_ref.py's: the recurrence of
afm_mlp.h) and the fit over epochs with the per-epoch moments -- in a dtype of the caller's choice
(float64: what the kernels compute up to the order of addition and the last bits of exp / tanh;
longdouble: the value the bounds are taken around), with a choice of two summation orders (k
ascending, k descending) and, with ``ulps=k``, every sigmoid / tanh result moved by a seeded
integer in [-k, k] steps of np.nextafter: the spread of these runs around the longdouble one is
the tolerance of the device tests.  Every sum is a sequential loop in the stated order.

Designs here are host arrays X [n][T][d]; theta is the flat vector K1[d + H1][4 H1], b1[4 H1],
K2[H1 + H2][4 H2], b2[4 H2], w[H2], b3 with the gate blocks in the order i, f, g, o; a shape is
(T, d, H1, H2)."""
import numpy as np

from mlp_ref import LD, U, adam_state, adam_step, moments, moments_bound, seq_matmul  # noqa: F401

ACT_ULPS = 4          # the bound of the device sigmoid / tanh error in ulps (test_lstm_kernels_gpu)


def param_count(d, h1, h2):
    return (d + h1) * 4 * h1 + 4 * h1 + (h1 + h2) * 4 * h2 + 4 * h2 + h2 + 1


def blocks(d, h1, h2):
    """name -> slice of theta; K1 split into its input rows (K1x) and recurrent rows (K1h)."""
    out, o = {}, 0
    for name, k in (("K1x", d * 4 * h1), ("K1h", h1 * 4 * h1), ("b1", 4 * h1),
                    ("K2", (h1 + h2) * 4 * h2), ("b2", 4 * h2), ("w", h2), ("b3", 1)):
        out[name] = slice(o, o + k)
        o += k
    assert o == param_count(d, h1, h2)
    return out


def unpack(theta, d, h1, h2):
    o, out = 0, []
    for shape in ((d + h1, 4 * h1), (4 * h1,), (h1 + h2, 4 * h2), (4 * h2,), (h2,), (1,)):
        k = int(np.prod(shape))
        out.append(theta[o:o + k].reshape(shape))
        o += k
    assert o == len(theta)
    return out


class Acts:
    """sig(z) = 1.0 / (1.0 + exp(-z)) and tanh in ``dtype``; with ulps > 0 every result is moved by
    an integer in [-ulps, ulps] steps of nextafter drawn from default_rng(seed)."""

    def __init__(self, dtype, ulps=0, seed=0):
        self.dtype, self.ulps = dtype, ulps
        self.rng = np.random.default_rng(seed)

    def nudge(self, v):
        if not self.ulps:
            return v
        steps = self.rng.integers(-self.ulps, self.ulps + 1, size=v.shape)
        for k in range(1, self.ulps + 1):
            up, dn = steps >= k, steps <= -k
            v = np.where(up, np.nextafter(v, self.dtype(np.inf)),
                         np.where(dn, np.nextafter(v, self.dtype(-np.inf)), v))
        return v

    def sig(self, z):
        with np.errstate(over="ignore"):
            return self.nudge(self.dtype(1.0) / (self.dtype(1.0) + np.exp(-z)))

    def tanh(self, z):
        return self.nudge(np.tanh(z))


def layer_forward(K, b, xs, H, act, rev):
    """One layer over the steps: xs [T] of [n][din] -> lists (per step) of a, i, f, g, o, c, tc, h."""
    n, dtype = xs[0].shape[0], act.dtype
    h, c = np.zeros((n, H), dtype), np.zeros((n, H), dtype)
    out = {k: [] for k in ("a", "i", "f", "g", "o", "c", "tc", "h")}
    for x in xs:
        a = np.concatenate([x, h], axis=1)
        z = seq_matmul(a, K, rev) + b
        i, f = act.sig(z[:, :H]), act.sig(z[:, H:2 * H])
        g, o = act.tanh(z[:, 2 * H:3 * H]), act.sig(z[:, 3 * H:])
        c = f * c + i * g
        tc = act.tanh(c)
        h = o * tc
        for k, v in zip(out, (a, i, f, g, o, c, tc, h)):
            out[k].append(v)
    return out


def forward(theta, X, shape, dtype=np.float64, rev=False, ulps=0, seed=0, cache=False):
    """F of the rows of X [n][T][d] (and, with cache, the two layers' stored values)."""
    T, d, h1, h2 = shape
    K1, b1, K2, b2, w, b3 = unpack(np.asarray(theta, dtype=dtype), d, h1, h2)
    X = np.asarray(X, dtype=dtype).reshape(-1, T, d)
    act = Acts(dtype, ulps, seed)
    L1 = layer_forward(K1, b1, [X[:, t, :] for t in range(T)], h1, act, rev)
    L2 = layer_forward(K2, b2, L1["h"], h2, act, rev)
    F = seq_matmul(L2["h"][-1], w[:, None], rev)[:, 0] + b3[0]
    return (F, L1, L2) if cache else F


def layer_backward(K, L, H, dh_in, dtype, rev):
    """BPTT of one layer: dh_in [T] of [n][H] (or None for 0) -> g_K, g_b, dx [T] of [n][din]."""
    T, n = len(L["a"]), L["a"][0].shape[0]
    din = K.shape[0] - H
    one = dtype(1.0)
    dhn, dcn = np.zeros((n, H), dtype), np.zeros((n, H), dtype)
    dzs, dxs = [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        i, f, g, o, tc = (L[k][t] for k in ("i", "f", "g", "o", "tc"))
        cp = L["c"][t - 1] if t > 0 else np.zeros((n, H), dtype)
        dh = (dh_in[t] if dh_in[t] is not None else np.zeros((n, H), dtype)) + dhn
        do = dh * tc
        dc = (dh * o) * (one - tc * tc) + dcn
        di, dg, df = dc * g, dc * i, dc * cp
        dcn = dc * f
        dz = np.concatenate([(di * i) * (one - i), (df * f) * (one - f), dg * (one - g * g),
                             (do * o) * (one - o)], axis=1)
        dzs[t] = dz
        back = seq_matmul(dz, K.T, rev)
        dxs[t], dhn = back[:, :din], back[:, din:]
    # the sums over (t, row): t ascending (descending with rev), the rows in seq_matmul's order
    gK, gb = np.zeros(K.shape, dtype), np.zeros(4 * H, dtype)
    ones = np.ones((1, n), dtype)
    for t in (range(T - 1, -1, -1) if rev else range(T)):
        gK = gK + seq_matmul(L["a"][t].T, dzs[t], rev)
        gb = gb + seq_matmul(ones, dzs[t], rev)[0]
    return gK, gb, dxs


def gradient(theta, X, y, shape, dtype=np.float64, rev=False, ulps=0, seed=0):
    """The gradient of the batch's mean squared error as a flat vector in the theta order, and F."""
    T, d, h1, h2 = shape
    K1, b1, K2, b2, w, b3 = unpack(np.asarray(theta, dtype=dtype), d, h1, h2)
    y = np.asarray(y, dtype=dtype)
    nb = len(y)
    F, L1, L2 = forward(theta, X, shape, dtype, rev, ulps, seed, cache=True)
    dF = (F - y) * (dtype(2.0) / dtype(nb))
    g_w = seq_matmul(L2["h"][-1].T, dF[:, None], rev)[:, 0]
    g_b3 = seq_matmul(np.ones((1, nb), dtype), dF[:, None], rev)[0]
    dh2 = [None] * (T - 1) + [dF[:, None] * w[None, :]]
    gK2, gb2, dx2 = layer_backward(K2, L2, h2, dh2, dtype, rev)
    gK1, gb1, _ = layer_backward(K1, L1, h1, dx2, dtype, rev)
    return np.concatenate([gK1.ravel(), gb1, gK2.ravel(), gb2, g_w, g_b3]), F


def fit(theta0, X, y, n_train, n_eval, shape, *, lr, beta1=0.9, beta2=0.999, eps=1e-7, batch=256,
        epochs=1, dtype=np.float64, rev=False, ulps=0, seed=0):
    """One model's fit.  -> dict: theta, evals [epochs][2][6], snaps [epochs][P], steps (theta
    before every step), F_train [epochs][n_train] (the predictions each step made before its
    update), F_eval [epochs][n_eval]."""
    theta = np.asarray(theta0, dtype=dtype).copy()
    X, y = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)
    st = adam_state(len(theta), dtype)
    evals, snaps, steps, Ftr, Fev = [], [], [], [], []
    k = 0
    for _ in range(epochs):
        F = np.zeros(n_train, dtype=dtype)
        for i in range(0, n_train, batch):
            j = min(i + batch, n_train)
            steps.append(theta)
            g, F[i:j] = gradient(theta, X[i:j], y[i:j], shape, dtype, rev, ulps, seed + k)
            theta = adam_step(theta, g, st, lr, beta1, beta2, eps, dtype)
            k += 1
        if n_eval:
            Fe = forward(theta, X[n_train:n_train + n_eval], shape, dtype, rev, ulps, seed + k)
        else:
            Fe = np.zeros(0, dtype)
        evals.append([moments(F, y[:n_train]), moments(Fe, y[n_train:n_train + n_eval])])
        snaps.append(theta)
        Ftr.append(F)
        Fev.append(Fe)
    return {"theta": theta, "evals": np.array(evals), "snaps": np.array(snaps), "steps": steps,
            "F_train": np.array(Ftr), "F_eval": np.array(Fev)}


def variants():
    """The fp64 restatements whose distance from the longdouble run is the spread s."""
    return (dict(), dict(rev=True), dict(ulps=ACT_ULPS, seed=1))
