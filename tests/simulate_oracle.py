"""Independent float64 statement of posterior predictive simulation (``phk_simulate``, defined in ``include/phlash_hip.h``):
the structured draw rule stated with loops over sites and states, an independent dense sampler on
``oracle.psmc_numpy.dense_from_pp`` fed the same uniforms, the two statistics stated site by site, and the exact law of
(path, codes) by enumeration.  Test infrastructure only, CPU only; shares no code with ``phlash_amd/simulate.py``.

A sequence is (q, r): q = seq0 + b S + s numbers (particle, row) in the call, r the replicate.  The Philox block at counter
(t, r, q lo, q hi) gives U1_t (words 0, 1: the transition into site t) and U2_t (words 2, 3: the emission at site t); site
0xFFFFFFFF gives U0 for the state before site 0.  Every function here takes the sequences as arrays ``q``, ``r`` of one
length n; the uniforms are generated for all of them at once, the draws go one sequence and one site at a time, in float64
scalars (IEEE, one rounding per operation), in the order the header writes.

Margins.  Next to each draw the distance of its theta to the nearest boundary of the draw, relative to the draw's total:
``m_path [n, L]`` for the transition into the site, ``m_obs [n, L]`` for the emission, ``m_start [n]``.  The kernel evaluates
the same operations in the same order, so equality does not depend on the margins; they are there to diagnose a mismatch.
"""

from __future__ import annotations

import itertools

import numpy as np

from oracle.psmc_numpy import dense_from_pp
from sampling_oracle import philox4x32_10, u53

START_SITE = 0xFFFFFFFF


def serial_cumsum(x):
    """inclusive sums in ascending index, one rounding per addition"""
    out, acc = np.empty(len(x)), 0.0
    for k, v in enumerate(np.asarray(x, float)):
        acc = acc + float(v)
        out[k] = acc
    return out


def uniforms(seed, q, r, t):
    """(U1, U2) [n] of the sequences (q, r) at site ``t`` (an integer; START_SITE for the start)"""
    q = np.asarray(q, dtype=np.uint64)
    x = philox4x32_10((np.uint64(t), np.asarray(r, dtype=np.uint64), q & np.uint64(0xFFFFFFFF), q >> np.uint64(32)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    return u53(x[0], x[1]), u53(x[2], x[3])


def uniforms_all(seed, q, r, L):
    """(U1, U2) [L, n]: all sites of the sequences at once (the generator is counter-based)"""
    q = np.asarray(q, dtype=np.uint64)[None, :]
    r = np.asarray(r, dtype=np.uint64)[None, :]
    t = np.arange(L, dtype=np.uint64)[:, None]
    x = philox4x32_10((t, r, q & np.uint64(0xFFFFFFFF), q >> np.uint64(32)), (seed & 0xFFFFFFFF, seed >> 32))
    return u53(x[0], x[1]), u53(x[2], x[3])


def _mass(x):
    return np.isfinite(x) & (x > 0.0)


def simulate_paths(pp, L, q, r, seed, margins=True):
    """The hidden paths and the unmasked codes of the sequences (q [n], r [n]) under the block ``pp`` (``margins=False``: the
    margin arrays are left at zero, which is several times faster at K = 64).
    -> dict(paths uint8 [n, L], codes int8 [n, L] in {0, 1}, flag, m_start [n], m_path [n, L], m_obs [n, L])"""
    b, d, u, v, e0, e1, pi = (np.asarray(x, float) for x in pp)
    K = len(d)
    q, r = np.asarray(q), np.asarray(r)
    n = len(q)
    cp, cb, cv = serial_cumsum(pi), serial_cumsum(b), serial_cumsum(v)
    flag = False
    with np.errstate(all="ignore"):
        # ---- start
        U0, _ = uniforms(seed, q, r, START_SITE)
        if _mass(cp[K - 1]):
            th = U0 * cp[K - 1]
            z = np.zeros(n, int)
            for k in range(K - 1):
                z += cp[k] <= th
            m_start = np.abs(cp[None, :] - th[:, None]).min(1) / cp[K - 1]
        else:
            z, m_start, flag = np.zeros(n, int), np.zeros(n), True
        U1, U2 = uniforms_all(seed, q, r, L)
        paths = np.empty((n, L), np.uint8)
        codes = np.empty((n, L), np.int8)
        m_path, m_obs = np.zeros((n, L)), np.zeros((n, L))
        es = e0 + e1
        for t in range(L):
            for a in range(n):  # one sequence at a time: the definition, line by line
                i = int(z[a])
                PB = cb[i - 1] if i > 0 else 0.0
                SV = cv[K - 1] - cv[i]
                tot = PB + d[i] + u[i] * SV
                if _mass(tot):
                    theta = U1[t, a] * tot
                    if theta < PB:
                        j = sum(1 for k in range(i) if cb[k] <= theta)
                    else:
                        phi = theta - PB
                        if phi < d[i]:
                            j = i
                        else:
                            psi = phi - d[i]
                            j = min(K - 1, i + 1 + sum(1 for k in range(i + 1, K - 1) if u[i] * (cv[k] - cv[i]) <= psi))
                    if margins:
                        bounds = [cb[k] for k in range(i)] + [PB, PB + d[i]] + [PB + d[i] + u[i] * (cv[k] - cv[i]) for k in range(i + 1, K - 1)]
                        m_path[a, t] = min(abs(x - theta) for x in bounds) / tot
                else:
                    j, flag = i, True
                z[a] = j
                if _mass(es[j]):
                    x = U2[t, a] * es[j]
                    codes[a, t] = 1 if x < e1[j] else 0
                    m_obs[a, t] = abs(x - e1[j]) / es[j]
                else:
                    codes[a, t], flag = 0, True
            paths[:, t] = z
    return dict(paths=paths, codes=codes, flag=flag, m_start=m_start, m_path=m_path, m_obs=m_obs)


def lay_mask(codes, mask_row):
    """reported codes: -1 where the row's mask is negative"""
    out = np.array(codes, dtype=np.int8)
    if mask_row is not None:
        out[..., np.asarray(mask_row)[: out.shape[-1]] < 0] = -1
    return out


def statistics(obs, bin):
    """(het int32 [n, ceil(L / bin)], runs int32 [n, 32]) of reported codes obs [n, L], site by site: het counts the sites of
    a bin whose code is 1; runs is the histogram over floor(log2(len)) of the maximal runs of code 0, each counted when it
    ends (at a het, a missing site or the row's end)"""
    obs = np.asarray(obs)
    n, L = obs.shape
    het = np.zeros((n, -(-L // bin)), np.int32)
    runs = np.zeros((n, 32), np.int32)
    for a in range(n):
        run = 0
        for t in range(L):
            c = int(obs[a, t])
            if c == 1:
                het[a, t // bin] += 1
            if c == 0:
                run += 1
            elif run:
                runs[a, run.bit_length() - 1] += 1
                run = 0
        if run:
            runs[a, run.bit_length() - 1] += 1
    return het, runs


def simulate(pp, L, q, n_rep, seed, mask_row=None, bin=1):
    """One (particle, row) of a call: -> dict(obs int8 [n_rep, L], paths uint8 [n_rep, L], het, runs, flag, margins ...)"""
    out = simulate_paths(pp, L, np.full(n_rep, q), np.arange(n_rep), seed)
    out["obs"] = lay_mask(out["codes"], mask_row)
    out["het"], out["runs"] = statistics(out["obs"], bin)
    return out


def dense_simulate(pp, L, q, r, seed):
    """The same chain drawn from the DENSE matrix with the same uniforms: row-wise ``cumsum`` of ``dense_from_pp``, theta = U1
    times the row's last entry, state = #{k <= K-2 : C[i, k] <= theta}; start from cumsum(pi); the emission rule as defined.
    Not bit-equal to the structured rule (other sums, other roundings): a statistical cross-check.  -> (paths, codes)"""
    A = dense_from_pp(pp)
    K = A.shape[0]
    C = np.cumsum(A, axis=1)
    cp = np.cumsum(np.asarray(pp.pi, float))
    e0, e1 = np.asarray(pp.emis0, float), np.asarray(pp.emis1, float)
    q, r = np.asarray(q), np.asarray(r)
    U0, _ = uniforms(seed, q, r, START_SITE)
    z = (cp[None, : K - 1] <= (U0 * cp[-1])[:, None]).sum(1)
    U1, U2 = uniforms_all(seed, q, r, L)
    paths = np.empty((len(q), L), np.uint8)
    codes = np.empty((len(q), L), np.int8)
    for t in range(L):
        rows = C[z]
        z = (rows[:, : K - 1] <= (U1[t] * rows[:, -1])[:, None]).sum(1)
        paths[:, t] = z
        codes[:, t] = U2[t] * (e0[z] + e1[z]) < e1[z]
    return paths, codes


def exact_law(pp, L, masked=()):
    """{(path tuple, reported codes tuple): probability} over all K^L paths and 2^L codes (tiny K, L): start ~ pi / sum(pi),
    rows of the dense matrix normalised, het with probability emis1 / (emis0 + emis1); sites in ``masked`` report -1"""
    A = dense_from_pp(pp)
    A = A / A.sum(1, keepdims=True)
    pi = np.asarray(pp.pi, float) / np.sum(pp.pi)
    ph = np.asarray(pp.emis1, float) / (np.asarray(pp.emis0, float) + np.asarray(pp.emis1, float))
    K = len(pi)
    first = pi @ A  # the state at site 0
    law = {}
    for path in itertools.product(range(K), repeat=L):
        p = first[path[0]]
        for t in range(1, L):
            p *= A[path[t - 1], path[t]]
        for codes in itertools.product((0, 1), repeat=L):
            pc = p
            for t in range(L):
                pc *= ph[path[t]] if codes[t] else 1.0 - ph[path[t]]
            key = (path, tuple(-1 if t in masked else c for t, c in enumerate(codes)))
            law[key] = law.get(key, 0.0) + pc
    return law
