"""Independent float64 statement of posterior path sampling (``phk_sample_paths``): a normalised forward pass on the dense
transition matrix, the draw rule and the Philox4x32-10 uniforms of the definition in ``include/phlash_hip.h``, and the
comparators the CPU and GPU tests share.  Test infrastructure only, CPU only.

Conventions (``posterior_oracle``): alpha_0 = pi precedes site 0, alpha_t = (alpha_{t-1} A) .* e_{o_t} is the forward vector
after site t, a missing site has e = 1, the W warm-up sites condition the draw and are not reported.  The state at the last
site is drawn with weights alpha_{L-1}; the state at site t given state j at site t + 1 with weights alpha_t(i) A[i, j].  One
draw: c = inclusive prefix sum of the weights, theta = U c_{K-1}, state = #{i <= K - 2 : c_i <= theta}.  The margin of a draw
is min_i |c_i - theta| / c_{K-1}: how far theta is from the nearest boundary, i.e. how much relative error in the weights
the drawn state survives.
"""

from __future__ import annotations

import itertools

import numpy as np

from oracle.psmc_numpy import dense_from_pp

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four broadcastable integer arrays (32-bit words), key: two -> the four output words x0 .. x3 (uint64 arrays
    holding 32-bit values)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(*ctr)]
    k = [np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)]
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return c


def u53(x0, x1):
    """the float64 kernels' uniform"""
    return (np.asarray(x0, np.uint64) * np.uint64(1 << 21) + (np.asarray(x1, np.uint64) >> np.uint64(11))).astype(np.float64) * 2.0 ** -53


def u24(x0):
    """the float32 kernels' uniform: the top 24 bits of the same number"""
    return (np.asarray(x0, np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def uniforms(seed, q, r, t, bits24=False):
    """U of (seed, sequence q of the call, samples r [n], sites t [m]) -> float64 [m, n]"""
    r = np.asarray(r, dtype=np.uint64)[None, :]
    t = np.asarray(t, dtype=np.uint64)[:, None]
    x = philox4x32_10((t, r, np.uint64(q & 0xFFFFFFFF), np.uint64(q >> 32)), (seed & 0xFFFFFFFF, seed >> 32))
    return u24(x[0]) if bits24 else u53(x[0], x[1])


def _emis_rows(pp, real):
    return [np.asarray(pp.emis0, float).astype(real), np.asarray(pp.emis1, float).astype(real), np.ones(len(np.asarray(pp.pi)), real)]


def _codes(data):
    d = np.asarray(data).astype(int)
    return np.where(d < 0, 2, np.where(d >= 1, 1, 0))


def forward(pp, data, real=np.float64, W=None):
    """normalised alpha [L, K] (every array and operation in ``real``; the dense model is built in float64 and rounded once);
    with ``W`` also ll = log P(o) - log P(o_{<W}), what the forward kernel returns"""
    A = dense_from_pp(pp).astype(real)
    e = _emis_rows(pp, real)
    codes = _codes(data)
    a = np.asarray(pp.pi, float).astype(real)
    alpha = np.empty((len(codes), A.shape[0]), real)
    c = np.empty(len(codes), real)
    for t, code in enumerate(codes):
        a = (a @ A) * e[code]
        c[t] = a.sum(dtype=real)
        a = a / c[t]
        alpha[t] = a
    if W is None:
        return alpha
    return alpha, float(np.log(c[W:].astype(float)).sum())


def cdf_at(alpha_t, A, j, real=np.float64):
    """the normalised inclusive prefix sums of one draw's weights: state at a site with forward vector ``alpha_t`` given state
    ``j`` at the next site (``None``: the last site), in ``real``"""
    a = np.asarray(alpha_t, real)
    w = a if j is None else a * np.asarray(A, real)[:, j]
    c = np.cumsum(w, dtype=real)
    return c / c[-1]


def sample(pp, data, W, q, n_samples, seed, bits24=False, alpha=None):
    """-> (paths uint8 [n_samples, L - W], margins float64 [n_samples, L - W]) of sequence ``q`` of a call"""
    A = dense_from_pp(pp)
    if alpha is None:
        alpha = forward(pp, data)
    L, K = alpha.shape
    U = uniforms(seed, q, np.arange(n_samples), np.arange(L), bits24)  # [L, n]
    paths = np.empty((n_samples, L), np.uint8)
    margins = np.empty((n_samples, L))
    cur = None
    for t in range(L - 1, W - 1, -1):
        w = np.broadcast_to(alpha[t], (n_samples, K)) if cur is None else alpha[t][None, :] * A[:, cur].T
        c = np.cumsum(w, axis=1)
        theta = U[t] * c[:, -1]
        cur = (c[:, : K - 1] <= theta[:, None]).sum(1)
        paths[:, t] = cur
        margins[:, t] = np.abs(c - theta[:, None]).min(1) / c[:, -1]
    return paths[:, W:], margins[:, W:]


def structured_sample(pp, data, W, q, n_samples, seed, real=np.float64):
    """The draw the kernels make, stated with loops: the folded model (b, d, v) <- emis0 .* (b, d, v) with emission rows 1,
    emis1 / emis0, 1 / emis0, the O(K) forward step, the weights (u_i alpha_i) v_j / d_j alpha_j / b_j alpha_i, a serial prefix
    sum inside every lane of four states, the lanes' totals scanned, the total by a butterfly, and the per-lane counts added
    up.  Every operation in ``real``.  -> paths uint8 [n_samples, L - W]"""
    f = real
    e0 = np.asarray(pp.emis0, float)
    b, d, v = ((e0 * np.asarray(x, float)).astype(f) for x in (pp.b, pp.d, pp.v))
    u = np.asarray(pp.u, float).astype(f)
    rows = [np.ones(len(e0), f), (np.asarray(pp.emis1, float) / e0).astype(f), (1.0 / e0).astype(f)]
    K = len(e0)
    Kp = -(-K // 4) * 4  # padded to whole lanes: states of weight zero
    pad = lambda x, fill=0.0: np.concatenate([x, np.full(Kp - K, fill, f)])  # noqa: E731
    b, d, v, u = pad(b), pad(d), pad(v), pad(u)
    rows = [pad(r, 1.0) for r in rows]
    codes = _codes(data)
    L = len(codes)
    a = pad(np.asarray(pp.pi, float).astype(f))
    alpha = np.empty((L, Kp), f)
    for t in range(L):
        ua = u * a
        pre = np.concatenate([[f(0)], np.cumsum(ua, dtype=f)[:-1]])
        suf = np.concatenate([np.cumsum(a[::-1], dtype=f)[::-1][1:], [f(0)]])
        a = (d * a + v * pre + b * suf) * rows[codes[t]]
        a = a * f(2.0) ** -np.frexp(a.sum(dtype=f))[1]
        alpha[t] = a
    U = uniforms(seed, q, np.arange(n_samples), np.arange(L), bits24=f is np.float32).astype(f)
    R = Kp // 4
    paths = np.empty((n_samples, L), np.uint8)
    for r in range(n_samples):
        cur = None
        for t in range(L - 1, W - 1, -1):
            x = alpha[t]
            if cur is None:
                w = x.copy()
            else:
                k = np.arange(Kp)
                w = np.where(k < cur, (u * x) * v[cur], np.where(k == cur, d[cur], b[cur]) * x).astype(f)
            c = np.cumsum(w.reshape(R, 4), axis=1, dtype=f)  # serial inside a lane
            run = c[:, 3]
            off = np.concatenate([[f(0)], np.cumsum(run, dtype=f)[:-1]])
            tot = run.copy()
            while len(tot) > 1:  # butterfly
                tot = tot[0::2] + tot[1::2]
            theta = U[t, r] * tot[0]
            inc = (off[:, None] + c).reshape(-1)
            cur = int((inc[: Kp - 1] <= theta).sum())
            paths[r, t] = cur
    return paths[:, W:]


def forward_backward(pp, data):
    """-> (alpha [L, K], beta [L, K]) normalised per site: gamma_t ~ alpha_t .* beta_t"""
    A = dense_from_pp(pp)
    e = _emis_rows(pp, np.float64)
    codes = _codes(data)
    alpha = forward(pp, data)
    beta = np.empty_like(alpha)
    b = np.ones(A.shape[0])
    for t in range(len(codes) - 1, -1, -1):
        beta[t] = b
        b = A @ (e[codes[t]] * b)
        b = b / b.sum()
    return alpha, beta


def pair_posterior(pp, data, t):
    """xi [K, K]: P(z at site t = i, z at site t + 1 = j | o)"""
    A = dense_from_pp(pp)
    e = _emis_rows(pp, np.float64)
    codes = _codes(data)
    alpha, beta = forward_backward(pp, data)
    xi = alpha[t][:, None] * A * (e[codes[t + 1]] * beta[t + 1])[None, :]
    return xi / xi.sum()


def path_probabilities(pp, data, W=0):
    """{reported path (tuple of the states at sites W .. L - 1): posterior probability} by enumerating every hidden path z_0 .. z_L:
    tiny K and L only"""
    A = dense_from_pp(pp)
    e = _emis_rows(pp, np.float64)
    codes = _codes(data)
    pi = np.asarray(pp.pi, float)
    L, K = len(codes), len(pi)
    out, total = {}, 0.0
    for path in itertools.product(range(K), repeat=L + 1):
        p = pi[path[0]]
        for t in range(L):
            p *= A[path[t], path[t + 1]] * e[codes[t]][path[t + 1]]
        total += p
        key = path[1 + W :]
        out[key] = out.get(key, 0.0) + p
    return {k: v / total for k, v in out.items()}


# ------------------------------------------------------------------------------------------------- comparators
def frequency_score(freq, prob, N):
    """max |freq - prob| in units of 6 binomial standard errors of N draws (the variance floored at that of one expected count);
    a pass is < 1"""
    freq, prob = np.asarray(freq, float), np.asarray(prob, float)
    return float((np.abs(freq - prob) / (6.0 * np.sqrt(np.maximum(prob * (1.0 - prob), 1.0 / N) / N))).max())


def site_score(paths, gamma):
    """paths [N, n] against the per-site posteriors gamma [n, K]"""
    N, n = paths.shape
    K = gamma.shape[1]
    freq = np.stack([(paths == k).mean(0) for k in range(K)], 1)
    return frequency_score(freq, gamma, N)


def pair_score(paths, i, xi):
    """joint frequency of the states at columns i, i + 1 of paths [N, n] against xi [K, K]"""
    N, K = paths.shape[0], xi.shape[0]
    freq = np.zeros((K, K))
    np.add.at(freq, (paths[:, i].astype(int), paths[:, i + 1].astype(int)), 1.0 / N)
    return frequency_score(freq, xi, N)


def count_unequal(ref, cand):
    """float64 parity: the number of (sample, site) entries at which the candidate's paths differ from the oracle's"""
    ref, cand = np.asarray(ref), np.asarray(cand)
    assert ref.shape == cand.shape, (ref.shape, cand.shape)
    return int((ref != cand).sum())


def f32_divergences(pp, data, W, ref, margins, cand, floor, alpha64=None, alpha32=None):
    """float32 parity.  ``ref`` / ``margins``: the oracle's paths under the 24-bit uniforms [n, L - W]; ``cand``: the float32
    kernel's.  Two chains fed the same uniforms stay together until one draw falls on different sides of a boundary; after that
    they are two different (both valid) chains.  So each candidate path must equal the oracle's from the right up to the first
    differing site, and there the oracle's margin must be below max(floor, 5 x E), E = the largest difference between the CDF of
    that draw computed in float32 (``forward`` and ``cdf_at`` in float32) and in float64 -- what float32 keeps of this draw.
    -> (number of paths that diverged, list of (sample, site, margin, bar) of the violations)"""
    ref, cand = np.asarray(ref), np.asarray(cand)
    assert ref.shape == cand.shape, (ref.shape, cand.shape)
    A = dense_from_pp(pp)
    diverged, bad = 0, []
    for r in range(ref.shape[0]):
        d = np.nonzero(ref[r] != cand[r])[0]
        if d.size == 0:
            continue
        diverged += 1
        i = int(d[-1])  # column of the right-most differing site
        t = i + W
        if alpha64 is None:
            alpha64 = forward(pp, data)
        if alpha32 is None:
            alpha32 = forward(pp, data, np.float32)
        j = None if i == ref.shape[1] - 1 else int(ref[r, i + 1])
        E = float(np.abs(cdf_at(alpha32[t], A, j, np.float32).astype(float) - cdf_at(alpha64[t], A, j)).max())
        bar = max(floor, 5.0 * E)
        if not margins[r, i] < bar:
            bad.append((r, t, float(margins[r, i]), bar))
    return diverged, bad
