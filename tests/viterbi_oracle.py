"""Independent float64 statement of Viterbi decoding (``phk_viterbi``): max-product in the LOG domain on the DENSE transition
matrix, a scorer for a given path, and a path enumeration for tiny problems.  Test infrastructure only.  Deliberately another
algorithmic form than the kernels (dense, log domain, no scans, no folded factors, no rescaling).

Convention (the forward recursion of ``oracle.psmc_numpy.psmc_ll``): z_0 ~ pi precedes site 0, site t (0-based) is step
t + 1, a missing site has e = 1:

    (z*_0 .. z*_n) = argmax pi(z_0) prod_{t=1..n} A[z_{t-1}, z_t] e_{o_{t-1}}(z_t),     logp = log of that maximum.

The reported path is z*_{W+1} .. z*_n: the states at sites W .. n-1.  Ties go to the lowest predecessor index and the lowest
final state (``numpy.argmax`` returns the first maximum).
"""

from __future__ import annotations

import itertools
import math

import numpy as np

from oracle.psmc_numpy import dense_from_pp


def _log_tables(pp):
    """-> log A [K, K], log emission rows [3, K] indexed by code (0 hom, 1 het, 2 missing), log pi [K]"""
    with np.errstate(divide="ignore"):
        logA = np.log(dense_from_pp(pp))
        e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
        le = np.stack([np.log(e0), np.log(e1), np.zeros_like(e0)])
        lpi = np.log(pi)
    return logA, le, lpi


def _codes(data):
    d = np.asarray(data).astype(np.int64)
    return np.where(d < 0, 2, np.minimum(d, 1))


def _gap(cand):
    """smallest difference, over the columns, between the largest and the second largest entry of a column"""
    if cand.shape[0] < 2:
        return np.inf
    top = np.partition(cand, cand.shape[0] - 2, axis=0)[-2:]
    with np.errstate(invalid="ignore"):
        g = top[1] - top[0]
    g = g[np.isfinite(top[1])]  # (a column that is all -inf decides nothing)
    return float(g.min()) if g.size else np.inf


def viterbi(pp, data, W: int = 0, want_margin: bool = True):
    """-> (path uint8 [n - W], logp, margin).  ``margin``: the smallest gap, over all sites and states and the final choice,
    between the best and the second-best candidate (inf without ``want_margin``): the distance of the problem from a tie."""
    logA, le, lpi = _log_tables(pp)
    codes = _codes(data)
    n, K = len(codes), len(lpi)
    back = np.empty((n, K), dtype=np.uint8)
    ld = lpi.copy()
    margin = np.inf
    for t in range(n):
        cand = ld[:, None] + logA  # [from, to]
        arg = cand.argmax(0)
        back[t] = arg
        if want_margin:
            margin = min(margin, _gap(cand))
        ld = cand[arg, np.arange(K)] + le[codes[t]]
    z = int(ld.argmax())
    logp = float(ld[z])
    if want_margin:
        margin = min(margin, _gap(ld[:, None]))
    path = np.empty(n, dtype=np.uint8)
    for t in range(n - 1, -1, -1):
        path[t] = z
        z = int(back[t, z])
    return path[W:], logp, float(margin)


def path_terms(pp, data, path, W: int = 0):
    """Per-site terms [n - W] of the joint log probability of the observations and the hidden path ``path`` (states at sites
    W .. n-1), maximised over what ``path`` leaves open (z_0 and, with a warm-up, the states at sites 0 .. W-1): term 0 holds
    that maximum, the step into path[0] and its emission; term t the step path[t-1] -> path[t] and its emission."""
    logA, le, lpi = _log_tables(pp)
    codes = _codes(data)
    z = np.asarray(path).astype(np.int64)
    assert len(z) == len(codes) - W and len(z) > 0
    ld = lpi.copy()
    for t in range(W):  # max-product over the open prefix
        ld = (ld[:, None] + logA).max(0) + le[codes[t]]
    terms = le[codes[W:], z]
    terms[0] += (ld + logA[:, z[0]]).max()
    terms[1:] += logA[z[:-1], z[1:]]
    return terms


def path_logp(pp, data, path, W: int = 0):
    """Their sum: the joint log probability of a given path (two gathers and a correctly rounded sum: cheap at any length)."""
    return math.fsum(path_terms(pp, data, path, W))


def deficit(pp, data, best_path, path, W: int = 0):
    """log probability ``path`` gives up against ``best_path``, summed term by term: sites where the two paths agree
    contribute exactly 0, so the figure is free of the rounding of two long sums (1e-7 on a 3,000,001-site row)."""
    return math.fsum(path_terms(pp, data, best_path, W) - path_terms(pp, data, path, W))


def bruteforce(pp, data, W: int = 0):
    """The same by enumerating every hidden path z_0 .. z_n: tiny K and n only.  -> (path uint8 [n - W], logp)"""
    logA, le, lpi = _log_tables(pp)
    codes = _codes(data)
    n, K = len(codes), len(lpi)
    best, best_path = -np.inf, None
    for zs in itertools.product(range(K), repeat=n + 1):
        lp = lpi[zs[0]]
        for t in range(n):
            lp += logA[zs[t], zs[t + 1]] + le[codes[t], zs[t + 1]]
        if lp > best:
            best, best_path = lp, zs
    return np.asarray(best_path[1 + W :], dtype=np.uint8), float(best)
