"""The numpy restatement of include/afm_mlp.h: the network p -> h1 -> h2 -> 1, one Adam step, the
fit over epochs with the per-epoch moments -- in a dtype of the caller's choice (float64: what the
kernels compute up to the order of addition; longdouble: the value the bounds are taken around)
and with a choice of two summation orders (k ascending, k descending).  Every sum is a sequential
loop in the stated order, so the order is this file's and not a BLAS's.

Designs here are host arrays X [n][p] (row-major); theta is the flat vector W1[p][h1], b1[h1],
W2[h1][h2], b2[h2], w3[h2], b3."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def param_count(p, h1, h2):
    return p * h1 + h1 + h1 * h2 + h2 + h2 + 1


def unpack(theta, p, h1, h2):
    o, out = 0, []
    for shape in ((p, h1), (h1,), (h1, h2), (h2,), (h2,), (1,)):
        k = int(np.prod(shape))
        out.append(theta[o:o + k].reshape(shape))
        o += k
    assert o == len(theta)
    return out


def seq_matmul(A, B, rev=False):
    """A [n][K] @ B [K][m], the K terms added one after the other (k descending with rev)."""
    K = A.shape[1]
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.result_type(A, B))
    for k in (range(K - 1, -1, -1) if rev else range(K)):
        acc = acc + A[:, k, None] * B[None, k, :]
    return acc


def forward(theta, X, shape, dtype=np.float64, rev=False):
    """-> z1, a1, z2, a2, f of the rows of X."""
    p, h1, h2 = shape
    W1, b1, W2, b2, w3, b3 = unpack(np.asarray(theta, dtype=dtype), p, h1, h2)
    X = np.asarray(X, dtype=dtype)
    z1 = seq_matmul(X, W1, rev) + b1
    a1 = np.where(z1 > 0, z1, dtype(0))
    z2 = seq_matmul(a1, W2, rev) + b2
    a2 = np.where(z2 > 0, z2, dtype(0))
    f = seq_matmul(a2, w3[:, None], rev)[:, 0] + b3[0]
    return z1, a1, z2, a2, f


def gradient(theta, X, y, shape, dtype=np.float64, rev=False):
    """The gradient of the batch's mean squared error as a flat vector in the theta order, and f."""
    p, h1, h2 = shape
    W1, b1, W2, b2, w3, b3 = unpack(np.asarray(theta, dtype=dtype), p, h1, h2)
    X, y = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)
    nb = len(y)
    z1, a1, z2, a2, f = forward(theta, X, shape, dtype, rev)
    d = (f - y) * (dtype(2.0) / dtype(nb))
    ones = np.ones((nb, 1), dtype=dtype)
    g_w3 = seq_matmul(a2.T, d[:, None], rev)[:, 0]
    g_b3 = seq_matmul(ones.T, d[:, None], rev)[0]
    d2 = np.where(z2 > 0, d[:, None] * w3[None, :], dtype(0))
    g_W2 = seq_matmul(a1.T, d2, rev)
    g_b2 = seq_matmul(ones.T, d2, rev)[0]
    d1 = np.where(z1 > 0, seq_matmul(d2, W2.T, rev), dtype(0))
    g_W1 = seq_matmul(X.T, d1, rev)
    g_b1 = seq_matmul(ones.T, d1, rev)[0]
    return np.concatenate([g_W1.ravel(), g_b1, g_W2.ravel(), g_b2, g_w3, g_b3]), f


def adam_state(P, dtype=np.float64):
    return {"m": np.zeros(P, dtype), "v": np.zeros(P, dtype), "b1p": dtype(1.0), "b2p": dtype(1.0)}


def lr_t(st, lr, beta1, beta2, dtype=np.float64):
    """Advance the running powers and return the step's learning rate."""
    st["b1p"] = st["b1p"] * dtype(beta1)
    st["b2p"] = st["b2p"] * dtype(beta2)
    return (dtype(lr) * np.sqrt(dtype(1.0) - st["b2p"])) / (dtype(1.0) - st["b1p"])


def adam_step(theta, g, st, lr, beta1, beta2, eps, dtype=np.float64):
    step = lr_t(st, lr, beta1, beta2, dtype)
    c1, c2 = dtype(1.0) - dtype(beta1), dtype(1.0) - dtype(beta2)
    st["m"] = st["m"] + (g - st["m"]) * c1
    st["v"] = st["v"] + (g * g - st["v"]) * c2
    return theta - (step * st["m"]) / (np.sqrt(st["v"]) + dtype(eps))


def moments(F, y):
    """{n, sum F, sum y, sum F^2, sum y^2, sum F y} in the dtype of F."""
    F, y = np.asarray(F), np.asarray(y, dtype=F.dtype)
    if len(F) == 0:
        return np.zeros(6, dtype=F.dtype)
    return np.array([len(F), F.sum(), y.sum(), (F * F).sum(), (y * y).sum(), (F * y).sum()],
                    dtype=F.dtype)


def fit(theta0, X, y, n_train, n_eval, shape, *, lr, beta1=0.9, beta2=0.999, eps=1e-7, batch=256,
        epochs=1, dtype=np.float64, rev=False):
    """One model's fit.  -> dict: theta, evals [epochs][2][6], snaps [epochs][P], steps (theta
    before every step), F_train [epochs][n_train] (the predictions each step made before its
    update), F_eval [epochs][n_eval]."""
    theta = np.asarray(theta0, dtype=dtype).copy()
    X, y = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)
    st = adam_state(len(theta), dtype)
    evals, snaps, steps, Ftr, Fev = [], [], [], [], []
    for _ in range(epochs):
        F = np.zeros(n_train, dtype=dtype)
        for i in range(0, n_train, batch):
            j = min(i + batch, n_train)
            steps.append(theta)
            g, F[i:j] = gradient(theta, X[i:j], y[i:j], shape, dtype, rev)
            theta = adam_step(theta, g, st, lr, beta1, beta2, eps, dtype)
        Fe = forward(theta, X[n_train:n_train + n_eval], shape, dtype, rev)[4]
        evals.append([moments(F, y[:n_train]), moments(Fe, y[n_train:n_train + n_eval])])
        snaps.append(theta)
        Ftr.append(F)
        Fev.append(Fe)
    return {"theta": theta, "evals": np.array(evals), "snaps": np.array(snaps), "steps": steps,
            "F_train": np.array(Ftr), "F_eval": np.array(Fev)}


def forward_bound(theta, X, shape):
    """(f, E) in longdouble: the forward value and a bound of the error of any fp64 evaluation of
    it that adds the K terms of a unit's sum and its bias in some order, one rounding per product
    and per add.  Such a sum of K + 1 terms carries at most gamma_(K+1) <= 2 (K + 1) u times the
    sum of the terms' magnitudes, and an input error E_in reaches the unit through |W|: per layer
    E_out = |W|' E_in + 2 (K + 1) u (|W|' |h| + |b|), E_0 = 0; relu moves no error up."""
    p, h1, h2 = shape
    W1, b1, W2, b2, w3, b3 = unpack(np.asarray(theta, dtype=LD), p, h1, h2)
    h, E = np.asarray(X, dtype=LD), np.zeros(np.shape(X), dtype=LD)
    for W, b, act in ((W1, b1, True), (W2, b2, True), (w3[:, None], b3, False)):
        K = W.shape[0]
        z = seq_matmul(h, W) + b
        E = seq_matmul(E, np.abs(W)) + 2 * (K + 1) * LD(U) * (seq_matmul(np.abs(h), np.abs(W))
                                                               + np.abs(b))
        h = np.where(z > 0, z, LD(0)) if act else z
    return h[:, 0], E[:, 0]


def forward_shift(theta, X, shape, tau):
    """A bound of |f(theta', x) - f(theta, x)| per row over every theta' within tau of theta in
    every entry (longdouble): per layer D_out = (|W| + tau)' D_in + tau (sum |h| + 1)."""
    p, h1, h2 = shape
    W1, b1, W2, b2, w3, b3 = unpack(np.asarray(theta, dtype=LD), p, h1, h2)
    h = np.asarray(X, dtype=LD)
    D = np.zeros(h.shape, dtype=LD)
    tau = LD(tau)
    for W, b, act in ((W1, b1, True), (W2, b2, True), (w3[:, None], b3, False)):
        z = seq_matmul(h, W) + b
        D = seq_matmul(D, np.abs(W) + tau) + tau * (np.abs(h).sum(axis=1, keepdims=True) + 1)
        h = np.where(z > 0, z, LD(0)) if act else z
    return D[:, 0]


def moments_bound(F, y, delta):
    """How far the six moments of predictions within delta of F (longdouble, row by row) summed in
    fp64 in any order can lie from moments(F, y): 2 n u sum |term| of the rounding, plus the
    change of every term."""
    F, y, delta = (np.asarray(a, dtype=LD) for a in (F, y, delta))
    n = len(F)
    if n == 0:
        return np.zeros(6, dtype=LD)
    aF = np.abs(F) + delta
    terms = [np.zeros(n, LD), aF, np.abs(y), aF * aF, y * y, aF * np.abs(y)]
    move = [np.zeros(n, LD), delta, np.zeros(n, LD), (2 * np.abs(F) + delta) * delta,
            np.zeros(n, LD), np.abs(y) * delta]
    return np.array([2 * (n + 2) * LD(U) * t.sum() + m.sum() for t, m in zip(terms, move)], dtype=LD)


def exact_grid(p, h1, h2, n, seed):
    """A design and a model on which every product and sum up to the gradients is exact in fp64:
    X integers in [-4, 4], y multiples of 1/8 in [-1, 1], W and w3 multiples of 1/8 in [-1/2,
    1/2], biases multiples of 1/4 in [-1/2, 1/2]."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-4, 5, size=(n, p)).astype(np.float64)
    y = rng.integers(-8, 9, size=n) / 8.0
    parts = [rng.integers(-4, 5, size=p * h1) / 8.0, rng.integers(-2, 3, size=h1) / 4.0,
             rng.integers(-4, 5, size=h1 * h2) / 8.0, rng.integers(-2, 3, size=h2) / 4.0,
             rng.integers(-4, 5, size=h2) / 8.0, rng.integers(-2, 3, size=1) / 4.0]
    return X, y, np.concatenate(parts)
