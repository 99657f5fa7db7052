"""Independent float64 statement of the transition posteriors (``phk_transitions``): the pair posterior xi_t on the dense
transition matrix, its split into arrivals (stay, up, down), masking by a row's own length, binning, and a path enumeration
for tiny problems.  Test infrastructure only; no code shared with the product.

Convention (``posterior_oracle``): z_0 ~ pi precedes site 0, alpha_t is the forward vector after site t (alpha_{-1} = pi),
beta_L = 1, a missing site has e = 1.  For a scored site t = W .. L-1,
    xi_t(i, j) = P(z_prev = i, z_t = j | o) = alpha_{t-1}(i) A[i, j] e_{o_t}(j) beta_t(j) / Z_t.

``structured`` states the same quantity the way the kernel forms it -- folded factors, running exclusive prefix and suffix,
one Z_t per site -- in plain loops over the states; its distance from the dense statement is the float64 rounding floor the
GPU bars are judged against.
"""

from __future__ import annotations

import itertools

import numpy as np

from oracle.psmc_numpy import dense_from_pp


def _emis(e0, e1, ob):
    if ob < 0:
        return np.ones_like(e0)
    return e1 if ob >= 1 else e0


def pair_posteriors(pp, data, W: int = 0):
    """-> (xi [L - W, K, K] of the scored sites, ll).  ``pp``: anything with fields b, d, u, v, emis0, emis1, pi."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = np.asarray(data).astype(int)
    L, K = len(data), len(pi)
    before = np.empty((L, K))  # alpha before site t, normalised
    c = np.empty(L)
    a = pi / pi.sum()
    c0 = pi.sum()
    for t in range(L):
        before[t] = a
        a = (a @ A) * _emis(e0, e1, data[t])
        c[t] = a.sum()
        a = a / c[t]
    xi = np.empty((L, K, K))
    b = np.ones(K)
    for t in range(L - 1, -1, -1):
        w = _emis(e0, e1, data[t]) * b
        x = before[t][:, None] * A * w[None, :]
        xi[t] = x / x.sum()
        b = A @ w
        b = b / b.sum()
    c[0] *= c0
    return xi[W:], float(np.log(c[W:]).sum())


def arrivals_of(xi):
    """xi [n, K, K] -> [n, 3, K]: (stay, up, down) per state reached -- the diagonal, and the column sums above and below it"""
    stay = np.einsum("tkk->tk", xi)
    up = np.triu(xi, 1).sum(1)
    down = np.tril(xi, -1).sum(1)
    return np.stack([stay, up, down], 1)


def reduce_bins(arr, W: int, bin: int, length: int | None = None):
    """arr [n, 3, K] of the scored sites W .. W + n - 1 -> (arrivals [nbin, 3, K], changes [nbin, 2]): per bin of ``bin``
    scored sites the MEAN of arr over the row's own sites (t < length) and the SUM of (sum_k up, sum_k down) over them; a bin
    without a site of the row's own is zeros."""
    n = arr.shape[0]
    length = W + n if length is None else length
    nb = (n + bin - 1) // bin
    A = np.zeros((nb,) + arr.shape[1:])
    C = np.zeros((nb, 2))
    for k in range(nb):
        lo, hi = k * bin, min((k + 1) * bin, n, length - W)
        if hi > lo:
            A[k] = arr[lo:hi].mean(0)
            C[k, 0] = arr[lo:hi, 1].sum()
            C[k, 1] = arr[lo:hi, 2].sum()
    return A, C


def transitions(pp, data, W: int = 0, bin: int = 1, length: int | None = None):
    """-> (arrivals [nbin, 3, K], changes [nbin, 2], ll) of one row"""
    xi, ll = pair_posteriors(pp, data, W)
    A, C = reduce_bins(arrivals_of(xi), W, bin, length)
    return A, C, ll


def bruteforce_pairs(pp, data, W: int = 0):
    """xi of the scored sites by enumerating every hidden path z_0 .. z_L: tiny K and L only."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = [int(o) for o in data]
    L, K = len(data), len(pi)
    xi = np.zeros((L, K, K))
    total = 0.0
    for path in itertools.product(range(K), repeat=L + 1):
        p = pi[path[0]]
        for t, ob in enumerate(data):
            p *= A[path[t], path[t + 1]] * _emis(e0, e1, ob)[path[t + 1]]
        total += p
        for t in range(L):
            xi[t, path[t], path[t + 1]] += p
    return xi[W:] / total


def structured(pp, data, W: int = 0):
    """-> arr [L - W, 3, K]: (stay, up, down) in the kernel's structured form, float64, loops over the states.

    The model is folded (column j of A carries the hom emission: b, d, v <- emis0 .* (b, d, v); a site multiplies by 1,
    emis1 / emis0 or 1 / emis0), the two running sums are the exclusive prefix of u .* alpha and the exclusive suffix of
    alpha, both of the alpha BEFORE the site, and every site is normalised by its own Z_t."""
    b, d, u, v, e0, e1, pi = (np.asarray(getattr(pp, f), float) for f in ("b", "d", "u", "v", "emis0", "emis1", "pi"))
    K = len(pi)
    bf, df, vf = e0 * b, e0 * d, e0 * v
    rows = (np.ones(K), e1 / e0, 1.0 / e0)  # hom, het, missing
    data = np.asarray(data).astype(int)
    L = len(data)

    def row(ob):
        return rows[2] if ob < 0 else rows[1 if ob >= 1 else 0]

    def scans(a):
        pre, suf = np.zeros(K), np.zeros(K)
        t = 0.0
        for k in range(K):
            pre[k] = t
            t += u[k] * a[k]
        t = 0.0
        for k in range(K - 1, -1, -1):
            suf[k] = t
            t += a[k]
        return pre, suf

    before = np.empty((L, K))
    pres = np.empty((L, K))
    sufs = np.empty((L, K))
    a = pi.copy()
    for t in range(L):
        pre, suf = scans(a)
        before[t], pres[t], sufs[t] = a, pre, suf
        a = (df * a + vf * pre + bf * suf) * row(data[t])
        a = a / a.sum()
    out = np.empty((L, 3, K))
    beta = np.ones(K)
    for t in range(L - 1, -1, -1):
        w = row(data[t]) * beta
        s = (df * before[t]) * w
        up = (vf * pres[t]) * w
        dn = (bf * sufs[t]) * w
        z = (s + up + dn).sum()
        out[t, 0], out[t, 1], out[t, 2] = s / z, up / z, dn / z
        # beta_{t-1}(i) = d_i w_i + sum_{j<i} b_j w_j + u_i sum_{j>i} v_j w_j
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
    return out[W:]
