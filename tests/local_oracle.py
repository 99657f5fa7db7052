"""Independent float64 statement of the local likelihood-ratio scan (``phk_local_ratio``): a second backward vector stepped
through the dense transition matrix and the emissions of an ALTERNATIVE model over a bin's sites, with a log scale of its own;
masking by a row's own length; and a path enumeration for tiny problems.  Test infrastructure only; no code shared with the
product.

Convention (``posterior_oracle`` / ``tract_oracle``): z_0 ~ pi precedes site 0, alpha_t is the forward vector after site t
(alpha_{-1} = pi), beta_{L-1} = 1 and beta_t holds the emissions of sites t+1 .. L-1 only, a missing site has e = 1 in both
models.  With (A, e) the fitted model and (A', e') the alternative (its pi is never used), bin k of the scored sites
s = W + k bin .. e = min(s + bin, L) - 1:
    q_e = beta_e,   q_{t-1} = A' (e'_{o_t} .* q_t) for t = e .. s,
    logratio_k = log sum_i alpha_{s-1}(i) q_{s-1}(i) - log sum_i alpha_{s-1}(i) beta_{s-1}(i).
A site at or past the row's own length is stepped with the fitted model; a bin without a site of the row's own is 0.

``structured`` states the same quantity the way the kernel forms it -- folded factors per model, the running sums of the
adjoint mat-vec, a power-of-two rescale of beta and an integer exponent of q's own relative to it -- in plain loops over the
states; its distance from the dense statement is the float64 rounding floor the GPU bars are judged against.
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


def _unpack(alts, bin):
    one_alt = hasattr(alts, "emis0")
    alts = [alts] if one_alt else list(alts)
    bins = (bin,) if np.isscalar(bin) else tuple(bin)
    return alts, one_alt, bins, np.isscalar(bin)


def _pack(out, one_alt, one_bin):
    out = [o[0] for o in out] if one_alt else out
    return out[0] if one_bin else out


def dense(pp, alt, data, W: int = 0, bin=1, length: int | None = None):
    """-> (logratio [nbin], ll).  ``pp`` / ``alt``: anything with fields b, d, u, v, emis0, emis1, pi.  A list of n alternatives
    gives [n, nbin]; a tuple of bin sizes gives a list with one such array per size (one backward pass for all of them).  q is
    kept normalised to its own sum, with the log of everything taken out of it relative to beta in ``lq``."""
    A = dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    alts, one_alt, bins, one_bin = _unpack(alt, bin)
    Aa = [dense_from_pp(a) for a in alts]
    ea = [(np.asarray(a.emis0, float), np.asarray(a.emis1, float)) for a in alts]
    data = np.asarray(data).astype(int)
    L, K = len(data), len(pi)
    length = L if length is None else int(length)
    al = np.empty((L + 1, K))  # al[t + 1] = alpha_t, normalised
    c = np.empty(L)
    al[0] = pi / pi.sum()
    for t in range(L):
        a = (al[t] @ A) * _emis(e0, e1, data[t])
        c[t] = a.sum()
        al[t + 1] = a / c[t]
    c[0] *= pi.sum()
    n = len(alts)
    out = [np.zeros((n, (L - W + bn - 1) // bn)) for bn in bins]
    last = [{e: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    first = [{s: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    b = np.ones(K)
    q = np.zeros((len(bins), n, K))
    lq = np.zeros((len(bins), n))
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(L - 1, W - 1, -1):
            for g in range(len(bins)):
                if t in last[g]:
                    q[g] = b
                    lq[g] = 0.0
            e = _emis(e0, e1, data[t])
            for j in range(n):
                if t < length:
                    q[:, j] = (_emis(ea[j][0], ea[j][1], data[t]) * q[:, j]) @ Aa[j].T
                else:
                    q[:, j] = (e * q[:, j]) @ A.T
            b = A @ (e * b)
            z = b.sum()
            b = b / z
            zq = q.sum(-1)
            q = np.where(zq[..., None] > 0, q / np.where(zq > 0, zq, 1.0)[..., None], 0.0)
            lq = lq + np.log(zq) - np.log(z)
            if t < length:
                for g in range(len(bins)):
                    if t in first[g]:
                        out[g][:, first[g][t]] = lq[g] + np.log(q[g] @ al[t]) - np.log(b @ al[t])
    return _pack(out, one_alt, one_bin), float(np.log(c[W:]).sum())


def bruteforce(pp, alt, data, W: int = 0, bin: int = 1, length: int | None = None):
    """logratio [nbin] from its definition, by enumerating every hidden path z_0 .. z_L at once: the probability of the data
    with the transition into and the emission of every own site of the bin taken from ``alt``, over that under ``pp``.  Tiny K
    and L only."""
    A, Aa = dense_from_pp(pp), dense_from_pp(alt)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    a0, a1 = np.asarray(alt.emis0, float), np.asarray(alt.emis1, float)
    data = [int(o) for o in data]
    L, K = len(data), len(pi)
    length = L if length is None else int(length)
    paths = np.indices((K,) * (L + 1)).reshape(L + 1, -1)  # [L + 1, K^(L+1)]: paths[t + 1] = z_t of every path

    def total(sites):
        p = pi[paths[0]].copy()
        for t, ob in enumerate(data):
            if t in sites:
                p *= Aa[paths[t], paths[t + 1]] * _emis(a0, a1, ob)[paths[t + 1]]
            else:
                p *= A[paths[t], paths[t + 1]] * _emis(e0, e1, ob)[paths[t + 1]]
        return p.sum()

    base = total(())
    out = []
    with np.errstate(divide="ignore"):
        for k, s, e in _bins(L, W, bin):
            if s >= length:
                out.append(0.0)
                continue
            out.append(float(np.log(total(range(s, min(e, length - 1) + 1)) / base)))
    return np.array(out)


RATIO_MIN_EMIS0 = 2.0**-64  # a model is folded when every entry of both emission rows is above this


class _Folded:
    """one model in the kernel's form: column j of A carries the hom emission (b, d, v <- emis0 .* (b, d, v); the table rows are
    1, emis1 / emis0 and 1 / emis0) where the ratios exist, else the factors and the emission rows as they are"""

    def __init__(self, pp):
        b, d, u, v, e0, e1 = (np.asarray(getattr(pp, f), float) for f in ("b", "d", "u", "v", "emis0", "emis1"))
        self.K = K = len(d)
        self.u = u
        if (e0 > RATIO_MIN_EMIS0).all() and (e1 > RATIO_MIN_EMIS0).all():
            self.b, self.d, self.v = e0 * b, e0 * d, e0 * v
            self.rows = (np.ones(K), e1 / e0, 1.0 / e0)  # hom, het, missing
        else:
            self.b, self.d, self.v = b, d, v
            self.rows = (e0, e1, np.ones(K))

    def row(self, ob):
        return self.rows[2] if ob < 0 else self.rows[1 if ob >= 1 else 0]

    def fwd(self, a, r):
        K = self.K
        out, pre = np.empty(K), np.empty(K)
        t = 0.0
        for k in range(K):
            pre[k] = t
            t += self.u[k] * a[k]
        t = 0.0
        for k in range(K - 1, -1, -1):
            out[k] = ((self.d[k] * a[k] + self.v[k] * pre[k]) + self.b[k] * t) * r[k]
            t += a[k]
        return out

    def back(self, w):
        """w [..., K]: the loops run over the states, every other axis rides along"""
        K = self.K
        out = np.empty_like(w)
        acc = np.zeros(w.shape[:-1])
        for i in range(K):
            out[..., i] = self.d[i] * w[..., i] + acc
            acc = acc + self.b[i] * w[..., i]
        acc = np.zeros(w.shape[:-1])
        for i in range(K - 1, -1, -1):
            out[..., i] += self.u[i] * acc
            acc = acc + self.v[i] * w[..., i]
        return out


def _exp_of(x):
    """the exponent frexp takes out of x, elementwise (0 for x = 0)"""
    return np.frexp(x)[1].astype(int)


def _log_scaled(r, qe):
    """log(r 2^qe): the exponent folded into the ratio while the product is a normal number, else added in the log domain"""
    m, er = np.frexp(r)
    E = er.astype(int) + qe
    with np.errstate(divide="ignore"):
        near = np.log(np.ldexp(m, np.clip(E, -1000, 1000)))
        far = np.log(m) + E * np.log(2.0)
    return np.where(np.abs(E) < 1000, near, far)


def structured(pp, alt, data, W: int = 0, bin=1, length: int | None = None):
    """-> logratio [nbin] in the kernel's structured form, float64, loops over the states (alternatives and bin sizes as
    ``dense``).

    Both models are folded, each by its own decision.  Forward (fitted model): alpha' = row .* (d' alpha + v' pre(u alpha) +
    b' suf(alpha)), rescaled by a power of two.  Backward, for beta on the fitted model's factors with w = row .* beta and for q
    on the alternative's with w = row' .* q: x_{t-1}(i) = d'_i w_i + sum_{j<i} b'_j w_j + u_i sum_{j>i} v'_j w_j.  beta is
    rescaled by the power of two of its own sum and q by that of ITS own sum; the integer qe collects the difference of the two
    exponents.  At a bin's first site the two sums against the alpha before it, their ratio times 2^qe, and the log."""
    F = _Folded(pp)
    alts, one_alt, bins, one_bin = _unpack(alt, bin)
    FA = [_Folded(a) for a in alts]
    pi = np.asarray(pp.pi, float)
    K = len(pi)
    data = np.asarray(data).astype(int)
    L = len(data)
    length = L if length is None else int(length)

    def dot(a, x):
        t = np.zeros(x.shape[:-1])
        for k in range(K):
            t = t + a[k] * x[..., k]
        return t

    al = np.empty((L + 1, K))
    al[0] = pi
    for t in range(L):
        a = F.fwd(al[t], F.row(data[t]))
        al[t + 1] = np.ldexp(a, -int(_exp_of(a.sum())))
    G, n = len(bins), len(alts)
    out = [np.zeros((n, (L - W + bn - 1) // bn)) for bn in bins]
    last = [{e: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    first = [{s: k for k, s, e in _bins(L, W, bn)} for bn in bins]
    beta = np.ones(K)
    q = np.zeros((G, n, K))
    qe = np.zeros((G, n), dtype=int)
    for t in range(L - 1, W - 1, -1):
        for g in range(G):
            if t in last[g]:
                q[g] = beta
                qe[g] = 0
        beta = F.back(F.row(data[t]) * beta)
        ex = int(_exp_of(dot(np.ones(K), beta)))
        beta = np.ldexp(beta, -ex)
        if t < length:
            for j in range(n):
                q[:, j] = FA[j].back(FA[j].row(data[t]) * q[:, j])
            xq = _exp_of(dot(np.ones(K), q))
            q = np.ldexp(q, -xq[..., None])
            qe = qe + xq - ex
        else:  # (padding lies to the right of a bin's own sites: q is beta there)
            q[:] = beta
            qe[:] = 0
        if t < length and any(t in f for f in first):
            den = dot(al[t], beta)
            num = dot(al[t], q)  # [G, n]
            for g in range(G):
                if t in first[g]:
                    out[g][:, first[g][t]] = _log_scaled(num[g] / den, qe[g])
    return _pack(out, one_alt, one_bin)
