"""Independent float64 statement of posterior decoding (``phk_posterior``): the textbook scaled forward-backward on the
dense transition matrix, and a path enumeration for tiny problems.  Test infrastructure only.

Convention (the forward recursion of ``oracle.psmc_numpy.psmc_ll``): alpha_0 = pi, alpha_t = (alpha_{t-1} A) .* e_{o_t},
beta_L = 1, beta_{t-1} = A (e_{o_t} .* beta_t), gamma_t = alpha_t .* beta_t / sum, a missing site has e = 1.  Site t of a
row (0-based) is the t+1-th step.  With a warm-up of W sites the posterior conditions on the whole row; only sites
W .. L-1 are reported, and ll = log P(o) - log P(o_{<W}) is what the forward kernel returns.
"""

from __future__ import annotations

import itertools
import math

import numpy as np

from oracle.psmc_numpy import dense_from_pp


def _emis(e0, e1, ob):
    if ob < 0:
        return np.ones_like(e0)
    return e1 if ob >= 1 else e0


def forward_backward(pp, data, W: int = 0):
    """-> (gamma [L - W, K] of the scored sites, ll).  ``pp``: anything with fields b, d, u, v, emis0, emis1, pi."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = np.asarray(data).astype(int)
    L, K = len(data), len(pi)
    alpha = np.empty((L, K))
    c = np.empty(L)
    a = pi.copy()
    for t in range(L):
        a = (a @ A) * _emis(e0, e1, data[t])
        c[t] = a.sum()
        a = a / c[t]
        alpha[t] = a
    gamma = np.empty((L, K))
    b = np.ones(K)
    for t in range(L - 1, -1, -1):
        g = alpha[t] * b
        gamma[t] = g / g.sum()
        b = A @ (_emis(e0, e1, data[t]) * b)
        b = b / b.sum()
    ll = float(np.log(c[W:]).sum())
    return gamma[W:], ll


def bin_means(x, bin: int):
    """[n, ...] -> [ceil(n / bin), ...]: means over consecutive groups of ``bin`` rows (the last group may be shorter)."""
    n = x.shape[0]
    nb = (n + bin - 1) // bin
    return np.stack([x[k * bin : min((k + 1) * bin, n)].mean(0) for k in range(nb)]) if nb else x[:0]


def bruteforce(pp, data, W: int = 0):
    """The same by enumerating every hidden path z_0 .. z_L (z_0 ~ pi precedes site 0): tiny K and L only."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = [int(o) for o in data]
    L, K = len(data), len(pi)
    post = np.zeros((L, K))
    total = 0.0
    prefix = 0.0  # P(o_{<W})
    for path in itertools.product(range(K), repeat=L + 1):
        p = pi[path[0]]
        for t, ob in enumerate(data):
            p *= A[path[t], path[t + 1]] * _emis(e0, e1, ob)[path[t + 1]]
        total += p
        for t in range(L):
            post[t, path[t + 1]] += p
    if W > 0:
        for path in itertools.product(range(K), repeat=W + 1):
            p = pi[path[0]]
            for t in range(W):
                p *= A[path[t], path[t + 1]] * _emis(e0, e1, data[t])[path[t + 1]]
            prefix += p
        ll = math.log(total) - math.log(prefix)
    else:
        ll = math.log(total)
    return post[W:] / total, ll
