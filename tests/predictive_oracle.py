"""Independent float64 statement of leave-one-out predictive decoding (``phk_predictive``): the cavity weight on the dense
transition matrix, the per-site het probability and log score, masking by a row's own length, binning, and a path enumeration
for tiny problems.  Test infrastructure only; no code shared with the product.

Convention (``posterior_oracle`` / ``transition_oracle``): z_0 ~ pi precedes site 0, alpha_{t-1} is the forward vector before
site t (alpha_{-1} = pi), beta_L = 1 and beta_t holds the emissions of sites t+1 .. L-1 only, a missing site has e = 1.  For a
scored site t = W .. L-1,
    c_t(k) = (alpha_{t-1} A)(k) beta_t(k),   n0_t = sum_k c_t(k) emis0(k),   n1_t = sum_k c_t(k) emis1(k),
    phet_t = n1_t / (n0_t + n1_t),   score_t = log(n_{o_t} / (n0_t + n1_t)) at an observed site, 0 at a missing one.

``structured`` states the same quantity the way the kernel forms it -- folded factors, running exclusive prefix and suffix,
the table's hom and het rows, one ratio per site -- in plain loops over the states; its distance from the dense statement is
the float64 rounding floor the GPU bars are judged against.
"""

from __future__ import annotations

import itertools

import numpy as np

from oracle.psmc_numpy import dense_from_pp


def _emis(e0, e1, ob):
    if ob < 0:
        return np.ones_like(e0)
    return e1 if ob >= 1 else e0


def _score(n0, n1, ob):
    if ob < 0:
        return 0.0
    return float(np.log((n1 if ob >= 1 else n0) / (n0 + n1)))


def loo(pp, data, W: int = 0):
    """-> (phet [L - W], score [L - W] of the scored sites, ll).  ``pp``: anything with fields b, d, u, v, emis0, emis1, pi."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = np.asarray(data).astype(int)
    L, K = len(data), len(pi)
    pred = np.empty((L, K))  # alpha_{t-1} A, normalised
    c = np.empty(L)
    a = pi / pi.sum()
    c0 = pi.sum()
    for t in range(L):
        pred[t] = a @ A
        a = pred[t] * _emis(e0, e1, data[t])
        c[t] = a.sum()
        a = a / c[t]
    phet, score = np.empty(L), np.empty(L)
    b = np.ones(K)
    for t in range(L - 1, -1, -1):
        cav = pred[t] * b
        n0, n1 = float(cav @ e0), float(cav @ e1)
        phet[t] = n1 / (n0 + n1)
        score[t] = _score(n0, n1, data[t])
        b = A @ (_emis(e0, e1, data[t]) * b)
        b = b / b.sum()
    c[0] *= c0
    return phet[W:], score[W:], float(np.log(c[W:]).sum())


def reduce_bins(phet, score, data, W: int, bin: int, length: int | None = None):
    """phet, score [n] of the scored sites W .. W + n - 1 of the row ``data`` -> track [nbin, 3]: per bin of ``bin`` scored
    sites the SUMS over the row's own sites (t < length) of (phet at observed sites, phet at missing sites, score); a bin without
    a site of the row's own is zeros."""
    n = phet.shape[0]
    obs = np.asarray(data)[W : W + n] >= 0
    length = W + n if length is None else length
    nb = (n + bin - 1) // bin
    T = np.zeros((nb, 3))
    for k in range(nb):
        lo, hi = k * bin, min((k + 1) * bin, n, length - W)
        if hi > lo:
            T[k, 0] = phet[lo:hi][obs[lo:hi]].sum()
            T[k, 1] = phet[lo:hi][~obs[lo:hi]].sum()
            T[k, 2] = score[lo:hi].sum()  # (0 at the missing sites already)
    return T


def predictive(pp, data, W: int = 0, bin: int = 1, length: int | None = None):
    """-> (track [nbin, 3], ll) of one row"""
    phet, score, ll = loo(pp, data, W)
    return reduce_bins(phet, score, data, W, bin, length), ll


def _path_total(A, e0, e1, pi, data):
    """P(o) by enumerating every hidden path z_0 .. z_L"""
    K, L = len(pi), len(data)
    total = 0.0
    for path in itertools.product(range(K), repeat=L + 1):
        p = pi[path[0]]
        for t, ob in enumerate(data):
            p *= A[path[t], path[t + 1]] * _emis(e0, e1, ob)[path[t + 1]]
        total += p
    return total


def bruteforce_loo(pp, data, W: int = 0):
    """phet and score of the scored sites from their definition as probabilities of whole rows, each by path enumeration:
    phet_t = P(o with o_t := het) / (P(o with o_t := hom) + P(o with o_t := het)).  Tiny K and L only."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = [int(o) for o in data]
    L = len(data)
    phet, score = np.empty(L), np.empty(L)
    for t in range(W, L):
        p0 = _path_total(A, e0, e1, pi, data[:t] + [0] + data[t + 1 :])
        p1 = _path_total(A, e0, e1, pi, data[:t] + [1] + data[t + 1 :])
        phet[t] = p1 / (p0 + p1)
        score[t] = _score(p0, p1, data[t])
    return phet[W:], score[W:]


def structured(pp, data, W: int = 0):
    """-> (phet [L - W], score [L - W]) in the kernel's structured form, float64, loops over the states.

    The model is folded (column j of A carries the hom emission: b, d, v <- emis0 .* (b, d, v); the table rows are 1,
    emis1 / emis0 and 1 / emis0), the two running sums are the exclusive prefix of u .* alpha and the exclusive suffix of alpha,
    both of the alpha BEFORE the site, the cavity weight is (d' alpha + v' pre + b' suf) .* beta, and n0 and n1 are its sums
    against the table's hom and het rows as they are."""
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

    pred = np.empty((L, K))
    a = pi.copy()
    for t in range(L):
        pre, suf = scans(a)
        pred[t] = (df * a + vf * pre) + bf * suf
        a = pred[t] * row(data[t])
        a = a / a.sum()
    phet, score = np.empty(L), np.empty(L)
    beta = np.ones(K)
    for t in range(L - 1, -1, -1):
        cav = pred[t] * beta
        n0, n1 = 0.0, 0.0
        for k in range(K):
            n0 += cav[k] * rows[0][k]
            n1 += cav[k] * rows[1][k]
        it = 1.0 / (n0 + n1)
        phet[t] = n1 * it
        score[t] = 0.0 if data[t] < 0 else float(np.log((n1 if data[t] >= 1 else n0) * it))
        w = row(data[t]) * beta
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
    return phet[W:], score[W:]
