"""Independent float64 statement of the pair counts (``phk_pair_counts``): the pair posterior of ``transition_oracle`` summed
over a row's own scored sites, C(i, j) = sum_t P(z_{t-1} = i, z_t = j | o), origin state first.  Test infrastructure only; no
code shared with the product.

``loop_form`` states the same matrix the way the kernel forms it -- folded factors, the raw outer products
G(i, j) = sum_t alpha_{t-1}(i) w_t(j) / Z_t with Z_t from the three structured products, A applied once at the end -- in plain
loops over the states; its distance from the dense statement is the float64 rounding floor the GPU bars are judged against.
"""

from __future__ import annotations

import numpy as np

import transition_oracle as to


def pair_counts(pp, data, W: int = 0, length: int | None = None):
    """-> (C [K, K], ll) of one row: xi_t summed over the scored sites W <= t < length (the row's own; default: all)"""
    xi, ll = to.pair_posteriors(pp, data, W)
    n = xi.shape[0] if length is None else length - W
    return xi[:n].sum(0), ll


def loop_form(pp, data, W: int = 0, length: int | None = None):
    """-> C [K, K] in the kernel's form, float64, loops over the states"""
    b, d, u, v, e0, e1, pi = (np.asarray(getattr(pp, f), float) for f in ("b", "d", "u", "v", "emis0", "emis1", "pi"))
    K = len(pi)
    bf, df, vf = e0 * b, e0 * d, e0 * v  # the folded factors: column j of A carries the hom emission
    rows = (np.ones(K), e1 / e0, 1.0 / e0)  # hom, het, missing
    data = np.asarray(data).astype(int)
    L = len(data)
    length = L if length is None else length

    def row(ob):
        return rows[2] if ob < 0 else rows[1 if ob >= 1 else 0]

    before = np.empty((L, K))
    a = pi.copy()
    for t in range(L):
        before[t] = a
        pre, suf = np.zeros(K), np.zeros(K)
        acc = 0.0
        for k in range(K):
            pre[k] = acc
            acc += u[k] * a[k]
        acc = 0.0
        for k in range(K - 1, -1, -1):
            suf[k] = acc
            acc += a[k]
        a = (df * a + vf * pre + bf * suf) * row(data[t])
        a = a / a.sum()
    G = np.zeros((K, K))
    beta = np.ones(K)
    for t in range(L - 1, W - 1, -1):
        w = row(data[t]) * beta
        ap = before[t]
        suf = np.zeros(K)
        acc = 0.0
        for k in range(K - 1, -1, -1):
            suf[k] = acc
            acc += ap[k]
        z = 0.0
        pre = 0.0
        for k in range(K):  # Z_t: the three structured products, summed over the states
            z += (df[k] * ap[k]) * w[k] + (vf[k] * pre) * w[k] + (bf[k] * suf[k]) * w[k]
            pre += u[k] * ap[k]
        if t < length:
            for i in range(K):
                G[i] += (ap[i] / z) * w  # (row i of the outer product)
        nb = np.empty(K)
        acc = 0.0
        for i in range(K):
            nb[i] = df[i] * w[i] + acc
            acc += bf[i] * w[i]
        acc = 0.0
        for i in range(K - 1, -1, -1):
            nb[i] += u[i] * acc
            acc += vf[i] * w[i]
        beta = nb / nb.sum()
    C = np.empty((K, K))
    for i in range(K):
        for j in range(K):
            C[i, j] = G[i, j] * (bf[j] if i > j else df[j] if i == j else u[i] * vf[j])
    return C


def error(c, ref):
    """the tests' metric: max over the entries of |C - oracle| / max(1, oracle)"""
    c, ref = np.asarray(c, float), np.asarray(ref, float)
    return float((np.abs(c - ref) / np.maximum(1.0, ref)).max())
