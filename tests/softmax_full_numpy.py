"""float64 restatement of the full softmax over the catalogue (csrc/softmax_full.hip, ops.softmax_full_rows /
softmax_full_cols, MatrixFactorization.softmax_nll):

    z[b, i] = <X[b], Q[i]>,  lse[b] = log sum_i exp(z[b, i]),  nll[b] = lse[b] - z[b, t_b],
    G[b, i] = g_b (exp(z[b, i] - lse[b]) - [i == t_b]),  dX = G Q,  dQ = G^T X

and the tolerances of the GPU tests, computed from the float64 reference of the fp32-rounded inputs."""
import numpy as np


def forward(X, Q, t):
    """(z, lse, nll) in float64"""
    X, Q = np.asarray(X, np.float64), np.asarray(Q, np.float64)
    z = X @ Q.T
    m = z.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(axis=1))
    return z, lse, lse - z[np.arange(z.shape[0]), t]


def weights(z, lse, t, g):
    """G (B, I) for the upstream gradient g (B,)"""
    G = np.exp(z - lse[:, None])
    G[np.arange(z.shape[0]), t] -= 1.0
    return G * np.asarray(g, np.float64)[:, None]


def nll_grads(X, Q, t, g):
    """(nll, lse, dX, dQ) in float64"""
    X, Q = np.asarray(X, np.float64), np.asarray(Q, np.float64)
    z, lse, nll = forward(X, Q, t)
    G = weights(z, lse, t, g)
    return nll, lse, G @ Q, G.T @ X


def bounds(X, Q, t, g):
    """(lse, nll, dX, dQ) absolute bounds for fp32 kernels: the first two are the ``prob`` tolerance applied to the two
    terms of nll; a gradient element may be off by 1e-4 of the sum of the magnitudes it adds up, each G entry taken with
    the fp32 error of its score (1e-6 A, A = |X| |Q|^T) and, at the target, with the floor 0.01 |g_b| for the
    cancellation of softmax(z) Q - Q[t] when the target's probability approaches 1"""
    X, Q, g = np.asarray(X, np.float64), np.asarray(Q, np.float64), np.abs(np.asarray(g, np.float64))
    z, lse, _ = forward(X, Q, t)
    rows = np.arange(z.shape[0])
    g_abs = np.abs(weights(z, lse, t, g)) + 1e-6 * g[:, None] * (np.abs(X) @ np.abs(Q).T)
    g_abs[rows, t] += 0.01 * g
    return (1e-5 * np.abs(lse) + 1e-6, 1e-5 * (np.abs(lse) + np.abs(z[rows, t])) + 1e-6,
            1e-4 * (g_abs @ np.abs(Q)), 1e-4 * (g_abs.T @ np.abs(X)))
