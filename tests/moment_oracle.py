"""Independent float64 statement of bin moments (``phk_bin_moments``): the two extra backward vectors on the dense transition
matrix, masking by a row's own length, and a path enumeration for tiny problems.  Test infrastructure only; no code shared
with the product.

Convention (``tract_oracle``): z_0 ~ pi precedes site 0, alpha_t is the forward vector after site t (alpha_{-1} = pi),
beta_{L-1} = 1 and beta_t holds the emissions of sites t+1 .. L-1 only, a missing site has e = 1.  With a value row v in
[-1, 1]^K, bin k of the scored sites s = W + k bin .. e = min(s + bin, L) - 1:
    q1_e = q2_e = 0,   w0 = e_{o_t} .* beta_t,  w1 = e_{o_t} .* q1_t,  w2 = e_{o_t} .* q2_t,
    beta_{t-1} = A w0,   q1_{t-1} = A (w1 + v .* w0),   q2_{t-1} = A (w2 + 2 v .* w1 + v^2 .* w0)   for t = e .. s,
    m1_k = sum_i alpha_{s-1}(i) q1_{s-1}(i) / sum_i alpha_{s-1}(i) beta_{s-1}(i) = E[S_k | o],   m2_k likewise with q2 = E[S_k^2 | o],
    S_k = sum_{t=s..e} v(z_t).
A site at or past the row's own length is stepped with v = 0; a bin without a site of the row's own has m1 = m2 = 0.

``structured`` states the same quantities the way the kernel forms them -- folded factors, the running sums of the adjoint
mat-vec, one power-of-two rescale shared by beta, q1 and q2, the third argument as w2 + v .* (w1 + x1) -- in plain loops over
the states; its distance from the dense statement is the float64 rounding floor the GPU bars are judged against.
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


def _unpack(v, bin):
    v = np.asarray(v, float)
    bins = (bin,) if np.isscalar(bin) else tuple(bin)
    return np.atleast_2d(v), v.ndim == 1, bins, np.isscalar(bin)


def _pack(out, one_v, one_bin):
    out = [o[0] for o in out] if one_v else out
    return out[0] if one_bin else out


def dense(pp, data, v, W: int = 0, bin=1, length: int | None = None):
    """-> (m1 [nbin], m2 [nbin], ll).  ``pp``: anything with fields b, d, u, v, emis0, emis1, pi.  n value rows v [n, K] give
    [n, nbin]; a tuple of bin sizes gives lists with one such array per size (one backward pass for all of them)."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = np.asarray(data).astype(int)
    L, K = len(data), len(pi)
    length = L if length is None else int(length)
    V, one_v, bins, one_bin = _unpack(v, bin)
    al = np.empty((L + 1, K))  # al[t + 1] = alpha_t, normalised
    c = np.empty(L)
    al[0] = pi / pi.sum()
    for t in range(L):
        a = (al[t] @ A) * _emis(e0, e1, data[t])
        c[t] = a.sum()
        al[t + 1] = a / c[t]
    c[0] *= pi.sum()
    G, n = len(bins), V.shape[0]
    o1 = [np.zeros((n, (L - W + bn - 1) // bn)) for bn in bins]
    o2 = [np.zeros((n, (L - W + bn - 1) // bn)) for bn in bins]
    last = [{e: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    first = [{s: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    b = np.ones(K)
    q1 = np.zeros((G, n, K))
    q2 = np.zeros((G, n, K))
    for t in range(L - 1, W - 1, -1):
        for g in range(G):
            if t in last[g]:
                q1[g] = 0.0
                q2[g] = 0.0
        e = _emis(e0, e1, data[t])
        vt = V if t < length else np.zeros_like(V)
        w0, w1, w2 = e * b, e * q1, e * q2
        q1 = (w1 + vt * w0) @ A.T
        q2 = (w2 + 2.0 * vt * w1 + vt * vt * w0) @ A.T
        b = A @ w0
        z = b.sum()
        b, q1, q2 = b / z, q1 / z, q2 / z
        if t < length:
            for g in range(G):
                if t in first[g]:
                    den = b @ al[t]
                    o1[g][:, first[g][t]] = (q1[g] @ al[t]) / den
                    o2[g][:, first[g][t]] = (q2[g] @ al[t]) / den
    return _pack(o1, one_v, one_bin), _pack(o2, one_v, one_bin), float(np.log(c[W:]).sum())


def bruteforce(pp, data, v, W: int = 0, bin: int = 1, length: int | None = None):
    """(m1 [nbin], m2 [nbin]) from the definition, E[S | o] and E[S^2 | o] with S = sum_{t in bin, t < length} v(z_t), by
    enumerating every hidden path z_0 .. z_L at once.  Tiny K and L only."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = [int(o) for o in data]
    L, K = len(data), len(pi)
    length = L if length is None else int(length)
    v = np.asarray(v, float)
    paths = np.indices((K,) * (L + 1)).reshape(L + 1, -1)  # [L + 1, K^(L+1)]: paths[t + 1] = z_t of every path
    p = pi[paths[0]].copy()
    for t, ob in enumerate(data):
        p *= A[paths[t], paths[t + 1]] * _emis(e0, e1, ob)[paths[t + 1]]
    total = p.sum()
    m1, m2 = [], []
    for k, s, e in _bins(L, W, bin):
        S = np.zeros_like(p)
        for t in range(s, min(e, length - 1) + 1):
            S += v[paths[t + 1]]
        m1.append(float((p * S).sum() / total))
        m2.append(float((p * S * S).sum() / total))
    return np.array(m1), np.array(m2)


def structured(pp, data, v, W: int = 0, bin=1, length: int | None = None):
    """-> (m1, m2) in the kernel's structured form, float64, loops over the states (value rows and bin sizes as ``dense``).

    The model is folded (column j of A carries the hom emission: b, d, v <- emis0 .* (b, d, v); the table rows are 1,
    emis1 / emis0 and 1 / emis0).  Forward: alpha' = row .* (d' alpha + v' pre(u alpha) + b' suf(alpha)), rescaled by a power of
    two.  Backward, with w0 = row .* beta, w1 = row .* q1, w2 = row .* q2, x1 = w1 + val .* w0 and x2 = w2 + val .* (w1 + x1),
    for each of w0, x1, x2 alike: y_{t-1}(i) = d'_i x_i + sum_{j<i} b'_j x_j + u_i sum_{j>i} v'_j x_j; beta is rescaled by a power of
    two of its own sum and q1, q2 are multiplied by the same power.  At a bin's first site the three sums against the alpha
    before it, and the two ratios."""
    b, d, u, vv, e0, e1, pi = (np.asarray(getattr(pp, f), float) for f in ("b", "d", "u", "v", "emis0", "emis1", "pi"))
    K = len(pi)
    bf, df, vf = e0 * b, e0 * d, e0 * vv
    rows = (np.ones(K), e1 / e0, 1.0 / e0)  # hom, het, missing
    data = np.asarray(data).astype(int)
    L = len(data)
    length = L if length is None else int(length)
    V, one_v, bins, one_bin = _unpack(v, bin)

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
    G, n = len(bins), V.shape[0]
    o1 = [np.zeros((n, (L - W + bn - 1) // bn)) for bn in bins]
    o2 = [np.zeros((n, (L - W + bn - 1) // bn)) for bn in bins]
    last = [{e: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    first = [{s: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    # one array for the loops over the states: x[g] = q1 of bin size g, x[G + g] = its q2, one row per value row; x[2G] = beta in every row
    x = np.zeros((2 * G + 1, n, K))
    x[2 * G] = 1.0
    for t in range(L - 1, W - 1, -1):
        for g in range(G):
            if t in last[g]:
                x[g] = 0.0
                x[G + g] = 0.0
        w = row(data[t]) * x
        if t < length:
            x1 = w[:G] + V * w[2 * G]
            w[G : 2 * G] = w[G : 2 * G] + V * (w[:G] + x1)
            w[:G] = x1
        x = back(w)
        x = x * pow2(dot(np.ones(K), x[2 * G, 0]))
        if t < length and any(t in f for f in first):
            s = dot(al[t], x)  # [2G + 1, n]
            for g in range(G):
                if t in first[g]:
                    o1[g][:, first[g][t]] = s[g] / s[2 * G]
                    o2[g][:, first[g][t]] = s[G + g] / s[2 * G]
    return _pack(o1, one_v, one_bin), _pack(o2, one_v, one_bin)
