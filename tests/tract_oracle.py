"""Independent float64 statement of tract posteriors (``phk_tracts``): the second backward vector on the dense transition
matrix, masking by a row's own length, and a path enumeration for tiny problems.  Test infrastructure only; no code shared
with the product.

Convention (``posterior_oracle`` / ``predictive_oracle``): z_0 ~ pi precedes site 0, alpha_t is the forward vector after site t
(alpha_{-1} = pi), beta_{L-1} = 1 and beta_t holds the emissions of sites t+1 .. L-1 only, a missing site has e = 1.  With a
weight row m in [0, 1]^K, bin k of the scored sites s = W + k bin .. e = min(s + bin, L) - 1:
    q_e = beta_e,   q_{t-1} = A (m .* e_{o_t} .* q_t) for t = e .. s,
    tract_k = sum_i alpha_{s-1}(i) q_{s-1}(i) / sum_i alpha_{s-1}(i) beta_{s-1}(i) = E[prod_{t=s..e} m(z_t) | o].
A site at or past the row's own length is stepped with m = 1; a bin without a site of the row's own is 0.

``structured`` states the same quantity the way the kernel forms it -- folded factors, the running sums of the adjoint
mat-vec, one power-of-two rescale shared by beta and q -- in plain loops over the states; its distance from the dense
statement is the float64 rounding floor the GPU bars are judged against.
"""

from __future__ import annotations

import numpy as np

from oracle.psmc_numpy import dense_from_pp


def _emis(e0, e1, ob):
    if ob < 0:
        return np.ones_like(e0)
    return e1 if ob >= 1 else e0


def _bins(L, W, bin):
    """[(k, s, e)] of the bins of the scored sites W .. L - 1"""
    nb = (L - W + bin - 1) // bin
    return [(k, W + k * bin, min(W + (k + 1) * bin, L) - 1) for k in range(nb)]


def _unpack(m, bin):
    m = np.asarray(m, float)
    bins = (bin,) if np.isscalar(bin) else tuple(bin)
    return np.atleast_2d(m), m.ndim == 1, bins, np.isscalar(bin)


def _pack(out, one_m, one_bin):
    out = [o[0] for o in out] if one_m else out
    return out[0] if one_bin else out


def dense(pp, data, m, W: int = 0, bin=1, length: int | None = None):
    """-> (tract [nbin], ll).  ``pp``: anything with fields b, d, u, v, emis0, emis1, pi.  n weight rows m [n, K] give
    [n, nbin]; a tuple of bin sizes gives a list with one such array per size (one backward pass for all of them)."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = np.asarray(data).astype(int)
    L, K = len(data), len(pi)
    length = L if length is None else int(length)
    M, one_m, bins, one_bin = _unpack(m, bin)
    al = np.empty((L + 1, K))  # al[t + 1] = alpha_t, normalised
    c = np.empty(L)
    al[0] = pi / pi.sum()
    for t in range(L):
        a = (al[t] @ A) * _emis(e0, e1, data[t])
        c[t] = a.sum()
        al[t + 1] = a / c[t]
    c[0] *= pi.sum()
    out = [np.zeros((M.shape[0], (L - W + bn - 1) // bn)) for bn in bins]
    last = [{e: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    first = [{s: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    b = np.ones(K)
    q = np.zeros((len(bins), M.shape[0], K))
    for t in range(L - 1, W - 1, -1):
        for g in range(len(bins)):
            if t in last[g]:
                q[g] = b
        e = _emis(e0, e1, data[t])
        q = ((M if t < length else 1.0) * e * q) @ A.T
        b = A @ (e * b)
        z = b.sum()
        b, q = b / z, q / z
        if t < length:
            for g in range(len(bins)):
                if t in first[g]:
                    out[g][:, first[g][t]] = (q[g] @ al[t]) / (b @ al[t])
    return _pack(out, one_m, one_bin), float(np.log(c[W:]).sum())


def bruteforce(pp, data, m, W: int = 0, bin: int = 1, length: int | None = None):
    """tract [nbin] from its definition, E[prod_{t in bin, t < length} m(z_t) | o], by enumerating every hidden path
    z_0 .. z_L at once.  Tiny K and L only."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = [int(o) for o in data]
    L, K = len(data), len(pi)
    length = L if length is None else int(length)
    m = np.asarray(m, float)
    paths = np.indices((K,) * (L + 1)).reshape(L + 1, -1)  # [L + 1, K^(L+1)]: paths[t + 1] = z_t of every path
    p = pi[paths[0]].copy()
    for t, ob in enumerate(data):
        p *= A[paths[t], paths[t + 1]] * _emis(e0, e1, ob)[paths[t + 1]]
    total = p.sum()
    out = []
    for k, s, e in _bins(L, W, bin):
        if s >= length:
            out.append(0.0)
            continue
        w = np.ones_like(p)
        for t in range(s, min(e, length - 1) + 1):
            w *= m[paths[t + 1]]
        out.append(float((p * w).sum() / total))
    return np.array(out)


def structured(pp, data, m, W: int = 0, bin=1, length: int | None = None):
    """-> tract [nbin] in the kernel's structured form, float64, loops over the states (weight rows and bin sizes as ``dense``).

    The model is folded (column j of A carries the hom emission: b, d, v <- emis0 .* (b, d, v); the table rows are 1,
    emis1 / emis0 and 1 / emis0).  Forward: alpha' = row .* (d' alpha + v' pre(u alpha) + b' suf(alpha)), rescaled by a power of
    two.  Backward, for beta with w = row .* beta and for q with w = (row .* m) .* q alike:
    x_{t-1}(i) = d'_i w_i + sum_{j<i} b'_j w_j + u_i sum_{j>i} v'_j w_j; beta is rescaled by a power of two of its own sum and q
    is multiplied by the same power.  At a bin's first site the two sums against the alpha before it, and their ratio."""
    b, d, u, v, e0, e1, pi = (np.asarray(getattr(pp, f), float) for f in ("b", "d", "u", "v", "emis0", "emis1", "pi"))
    K = len(pi)
    bf, df, vf = e0 * b, e0 * d, e0 * v
    rows = (np.ones(K), e1 / e0, 1.0 / e0)  # hom, het, missing
    data = np.asarray(data).astype(int)
    L = len(data)
    length = L if length is None else int(length)
    M, one_m, bins, one_bin = _unpack(m, bin)

    def row(ob):
        return rows[2] if ob < 0 else rows[1 if ob >= 1 else 0]

    def pow2(x):
        return np.ldexp(1.0, -int(np.frexp(x)[1]))

    def fwd(a, r):
        out = np.empty(K)
        t = 0.0
        pre = np.empty(K)
        for k in range(K):
            pre[k] = t
            t += u[k] * a[k]
        t = 0.0
        for k in range(K - 1, -1, -1):
            out[k] = ((df[k] * a[k] + vf[k] * pre[k]) + bf[k] * t) * r[k]
            t += a[k]
        return out

    def back(w):
        """w [..., K]: the loops run over the states, every other axis rides along"""
        out = np.empty_like(w)
        acc = np.zeros(w.shape[:-1])
        for i in range(K):
            out[..., i] = df[i] * w[..., i] + acc
            acc = acc + bf[i] * w[..., i]
        acc = np.zeros(w.shape[:-1])
        for i in range(K - 1, -1, -1):
            out[..., i] += u[i] * acc
            acc = acc + vf[i] * w[..., i]
        return out

    def dot(a, x):
        t = np.zeros(x.shape[:-1])
        for k in range(K):
            t = t + a[k] * x[..., k]
        return t

    al = np.empty((L + 1, K))
    al[0] = pi
    for t in range(L):
        a = fwd(al[t], row(data[t]))
        al[t + 1] = a * pow2(a.sum())
    out = [np.zeros((M.shape[0], (L - W + bn - 1) // bn)) for bn in bins]
    last = [{e: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    first = [{s: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    # one array for the loops over the states: x[g] = the q vectors of bin size g, one row per weight row; x[-1] = beta in every row
    G, n = len(bins), M.shape[0]
    x = np.zeros((G + 1, n, K))
    x[G] = 1.0
    for t in range(L - 1, W - 1, -1):
        for g in range(G):
            if t in last[g]:
                x[g] = x[G]
        r = row(data[t])
        w = np.empty_like(x)
        w[:G] = ((r * M) if t < length else r) * x[:G]
        w[G] = r * x[G]
        x = back(w)
        x = x * pow2(dot(np.ones(K), x[G, 0]))
        if t < length and any(t in f for f in first):
            s = dot(al[t], x)  # [G + 1, n]
            for g in range(G):
                if t in first[g]:
                    out[g][:, first[g][t]] = s[g] / s[G]
    return _pack(out, one_m, one_bin)
