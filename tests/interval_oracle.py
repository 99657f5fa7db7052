"""Independent float64 statement of interval tracts (``phk_interval_tracts``): a dense K x K transition matrix built here, one
backward pass per interval with a normalisation at every step and the logs summed, and a path enumeration for tiny problems.
Test infrastructure only; no code shared with the product, with ``tract_oracle`` or with ``local_oracle``.

Convention: z_0 ~ pi precedes site 0, alpha_t is the forward vector after site t (alpha_{-1} = pi), beta_{L-1} = 1 and beta_t
holds the emissions of sites t+1 .. L-1 only, a missing site has e = 1 and is restricted to the set like any other.  An interval
(start, end, S) in reported sites covers the sites s = W + start .. e = W + end - 1:
    q_e = beta_e,   q_{t-1} = A (1_S .* e_{o_t} .* q_t) for t = e .. s,
    logp = log sum_i alpha_{s-1}(i) q_{s-1}(i) - log sum_i alpha_{s-1}(i) beta_{s-1}(i) = log P(z_s .. z_e in S | o).
"""

from __future__ import annotations

import numpy as np


def transition(pp) -> np.ndarray:
    """A[i, j] = P(z_t = j | z_{t-1} = i): b_j below the diagonal, d_i on it, u_i v_j above"""
    b, d, u, v = (np.asarray(getattr(pp, f), float) for f in ("b", "d", "u", "v"))
    K = len(d)
    A = np.outer(u, v)
    low = np.tril_indices(K, -1)
    A[low] = np.broadcast_to(b, (K, K))[low]
    A[np.diag_indices(K)] = d
    return A


def _table(pp):
    e0, e1 = np.asarray(pp.emis0, float), np.asarray(pp.emis1, float)
    return {-1: np.ones_like(e0), 0: e0, 1: e1}


def as_set(S, K) -> np.ndarray:
    """a set as bool [K]: a boolean row, or an integer whose bit k says whether state k is inside"""
    if np.ndim(S) == 0:
        return np.array([(int(S) >> k) & 1 for k in range(K)], dtype=bool)
    S = np.asarray(S, dtype=bool)
    assert S.shape == (K,)
    return S


def dense(pp, data, W: int, intervals):
    """-> (logp [n], ll) for ``intervals`` = [(start, end, S), ...] in reported sites, any order, overlaps allowed (every interval
    is a pass of its own)"""
    A = transition(pp)
    pi = np.asarray(pp.pi, float)
    tab = _table(pp)
    obs = [int(np.sign(o)) for o in np.asarray(data).astype(int)]
    L, K = len(obs), len(pi)
    alpha = np.empty((L + 1, K))  # alpha[t + 1]: the direction of alpha_t
    alpha[0] = pi / pi.sum()
    ll = 0.0
    for t in range(L):
        a = (alpha[t] @ A) * tab[obs[t]]
        z = a.sum()
        alpha[t + 1] = a / z
        if t >= W:
            ll += np.log(z)
    beta = np.empty((L, K))  # the direction of beta_t
    beta[L - 1] = 1.0 / K
    for t in range(L - 1, 0, -1):
        x = A @ (tab[obs[t]] * beta[t])
        beta[t - 1] = x / x.sum()
    out = np.empty(len(intervals))
    for n, (start, end, S) in enumerate(intervals):
        s, e = W + int(start), W + int(end) - 1
        assert W <= s <= e < L
        ind = as_set(S, K).astype(float)
        q, bq = beta[e].copy(), beta[e].copy()
        lq = lb = 0.0
        for t in range(e, s - 1, -1):
            q = A @ (ind * tab[obs[t]] * q)
            bq = A @ (tab[obs[t]] * bq)
            zq, zb = q.sum(), bq.sum()
            if zq == 0.0:
                lq = -np.inf
                break
            q, bq = q / zq, bq / zb
            lq += np.log(zq)
            lb += np.log(zb)
        if np.isneginf(lq):
            out[n] = -np.inf
            continue
        num, den = alpha[s] @ q, alpha[s] @ bq
        out[n] = (lq + np.log(num)) - (lb + np.log(den)) if num > 0 else -np.inf
    return out, float(ll)


def bruteforce(pp, data, W: int, intervals):
    """logp [n] from its definition, by enumerating every hidden path z_0 .. z_L at once.  Tiny K and L only."""
    A = transition(pp)
    pi = np.asarray(pp.pi, float)
    tab = _table(pp)
    obs = [int(np.sign(o)) for o in np.asarray(data).astype(int)]
    L, K = len(obs), len(pi)
    paths = np.indices((K,) * (L + 1)).reshape(L + 1, -1)  # paths[t + 1] = z_t of every path
    p = pi[paths[0]].copy()
    for t, ob in enumerate(obs):
        p *= A[paths[t], paths[t + 1]] * tab[ob][paths[t + 1]]
    total = p.sum()
    out = []
    for start, end, S in intervals:
        inside = as_set(S, K)
        keep = np.ones(p.shape, dtype=bool)
        for t in range(W + int(start), W + int(end)):
            keep &= inside[paths[t + 1]]
        with np.errstate(divide="ignore"):
            out.append(float(np.log(p[keep].sum() / total)))
    return np.array(out)
