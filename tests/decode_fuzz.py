"""Seeded random draws for the decoding calls (``phk_posterior`` / ``phk_viterbi``), float32 emulations of their float64
oracles, and the comparators that hold a candidate output against the oracle.  Test infrastructure only, CPU only; used by
tests/test_decode_fuzz.py (the GPU tests and the CPU self-tests share the comparators) and tests/test_viterbi.py.

A draw holds everything a call depends on: K (compiled and padded sizes), float type, particles x chunks, chunk indices with
repeats into a kernel object of more rows, row length, warm-up, het / missing rates, runs of missing windows, broadcast or
really different per-chunk parameter blocks, rescale interval, workspace limit (both slab branches), and for posterior
decoding the plan, the bin, the values and which outputs are asked for; for Viterbi the rows' own lengths.

Bars.  Nothing here is measured on the kernels.
* float64 gamma: the project's flat F64_GAMMA_BAR.
* float32 gamma, per sequence: max(F32_GAMMA_BAR, 5 x E), E = the error of ``fb32`` (the oracle's dense forward-backward run
  in float32) on that sequence against the float64 oracle: the project's "5 x measured" rule applied to a figure measured on
  the reference.  E is taken per site (bin 1), over gamma and over the values-weighted mean scaled by max |values|: a bin
  mean of one float32 evaluation can cancel by chance, the per-site figure bounds every bin mean of it and measures what
  float32 keeps of this sequence (on an all-hom row the state sits at its fixed point and float32 drifts by 1e-5).
* Viterbi, per sequence: 0 <= deficit <= VITERBI_DEFICIT_ROUNDINGS x eps x n_diff, derived next to the constant.
"""

from __future__ import annotations

import functools
import math
import types

import numpy as np

import posterior_oracle as po
import viterbi_oracle as vo
from oracle import psmc_numpy as pn

KS = [4, 8, 16, 16, 32, 64, 5, 12, 20, 48]
LS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 64, 500, 511, 512, 513, 1025, 2600]
HETS = [0.0, 0.02, 0.1, 0.5]
MISSES = [0.0, 0.01, 0.3]
COMPILED_K = (4, 8, 16, 32, 64)
UNIT_SITES = 512  # sites per decode unit of a segmented plan

F64_GAMMA_BAR = 1e-10  # tests/test_posterior_decode.py
F32_GAMMA_BAR = 1.6e-5  # tests/test_posterior_decode.py: the floor of the per-sequence float32 bar
F32_REDRAW_BAR = 1e-3  # a float32 draw whose largest 5 x E exceeds this is redrawn as float64
F32_LOGP_BAR = 1e-5  # tests/test_viterbi.py
MIN_MARGIN = 1e-9  # tests/test_viterbi.py: exact path equality is asserted only this far from a tie
EPS = {False: 2.0 ** -24, True: 2.0 ** -53}  # unit roundoff by double_precision
# Viterbi deficit bound.  Split the reported sites into maximal stretches where the candidate's path differs from the
# oracle's: on a stretch the two paths are routes between the same two states, and the kernel took its own because, in ITS
# arithmetic, it scored at least as high.  A route's score is a product of one step per site; the step
#     delta'_j = e_j * max(v_j * max_{i<j}(u_i * delta_i), d_j * delta_j, b_j * max_{i>j} delta_i)
# carries at most c = 8 roundings per site along one route: the folded factor (b, d or v times emis0, rounded once: 1), u
# (rounded: 1), the emission ratio (emis1 / emis0 or 1 / emis0, rounded: 1), the products u_i * delta_i, v_j * (.), (.) * e_j
# (3; the d and b branches have fewer), which is 6, and 2 to spare for the rounding of pi and of the final comparison;
# rescaling by powers of two is exact.  Each rounding moves the log of a route's score by at most eps, so two routes of n
# steps that the kernel ranks the wrong way round differ by at most 2 c eps n in exact arithmetic: 16 eps n.
VITERBI_DEFICIT_ROUNDINGS = 16


# ------------------------------------------------------------------------------------------------- the draw
def _population(K, n, seed):
    """n valid models with K states: a sigma = 0.25 particle population as in the decode tests -> pn.PP, fields [n, K]"""
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population

    tmpl, x = particle_population(K, n, seed=seed, sigma=0.25)
    pp = PSMCParams.from_dm(tmpl.from_flat(x).to_dm())
    return pn.PP(*(np.asarray(a.numpy(), float) for a in pp))


def plan_lists(Kc, dbl):
    """the validity lists of test_random_shapes_against_the_oracle: forward / scan, serial sweep, segment sweep variants"""
    Rs = [r for r in (1, 2, 4, 8, 16) if r <= Kc and Kc // r <= (8 if dbl else 16)]
    Rsw = [r for r in Rs if Kc // r <= 4] if dbl else Rs
    Rsg = [r for r in Rs if Kc // r <= 4 or (Kc == 16 and Kc // r == 8)] if dbl else Rs
    return Rs, Rsw, Rsg


class Draw(types.SimpleNamespace):
    def block(self, b, s):
        """the parameter block of (particle b, chunk position s) as a pn.PP of [K] arrays"""
        return pn.PP(*(a[b, s if self.per_chunk else 0] for a in self.pp))

    def block_id(self, b, s):
        return (b, s if self.per_chunk else 0)

    def row_len(self, s):
        """the own length of the data row behind chunk position s"""
        return self.L if self.lens is None else int(self.lens[self.inds[s]])

    @property
    def nbin(self):
        return (self.L - self.W + self.bin - 1) // self.bin

    @property
    def n_units(self):
        """decode units of a segmented plan (phk_api.hip, n_units)"""
        T = self.plan[2]
        G = UNIT_SITES // T
        nblk = (self.L + T - 1) // T
        segW = ((self.W - 1) // T) // G if self.W > 0 else 0
        return (nblk + G - 1) // G - segW

    def bin_ends(self):
        """absolute site of every bin's last site"""
        return np.minimum(self.W + (np.arange(self.nbin) + 1) * self.bin, self.L) - 1

    def describe(self):
        s = (f"seed={self.seed} K={self.K} {'f64' if self.dbl else 'f32'}{'(redrawn)' if self.redrawn else ''} B={self.B} S={self.S} "
             f"N={self.N} inds={self.inds.tolist()} L={self.L} W={self.W} het={self.het} miss={self.miss} runs={int(self.runs)} "
             f"{'chunk' if self.per_chunk else 'bcast'} nrm={self.nrm} ws={self.ws} {'raw' if self.raw else 'api'}")
        if self.kind == "posterior":
            v = "none" if self.values is None else "x".join(map(str, self.values.shape))
            return s + f" plan={self.plan} bin={self.bin} values={v} marg={int(self.marginals)}"
        return s + f" lens={None if self.lens is None else self.lens.tolist()}"


STREAMS = {"posterior": 0, "viterbi": 1, "transitions": 2, "predictive": 3, "tracts": 4, "local": 5, "pairs": 6, "moments": 7}  # a random stream per kind


def _draw(seed, kind, force_dbl, with_rng=False):
    """Every kind but "viterbi" takes the posterior draw (the sweeps of tests/sweep_fuzz.py are dispatched as phk_posterior is);
    ``with_rng``: -> (draw, its generator), for a caller that draws more fields after these."""
    rng = np.random.default_rng([20_000 + seed, STREAMS[kind]])
    d = Draw(seed=seed, kind=kind, redrawn=False)
    # K x float type and the row length are stratified: every cell of the lists comes up within 20 resp. 16 seeds
    d.K = KS[seed % 10]
    d.Kc = min(k for k in COMPILED_K if k >= d.K)
    d.dbl = bool((seed // 10) % 2) or force_dbl
    d.L = L = LS[(5 * seed + seed // 16) % 16]
    d.B, d.S = int(rng.integers(1, 5)), int(rng.integers(1, 7))
    d.N = int(rng.integers(d.S, d.S + 5))
    d.inds = rng.integers(0, d.N, size=d.S)
    wmax = L - 1 if kind == "viterbi" else L
    d.W = int(rng.integers(0, wmax + 1)) if rng.integers(2) else 0
    edge = int(rng.integers(12))
    if edge == 0:
        d.W = L - 1
    elif edge == 1 and kind != "viterbi":
        d.W = L
    d.het = float(HETS[rng.integers(4)])
    d.miss = float(MISSES[rng.integers(3)])
    data = (rng.random((d.N, L)) < d.het).astype(np.int8)
    data[rng.random((d.N, L)) < d.miss] = -1
    d.runs = bool(rng.integers(3) == 0) and L >= 64
    if d.runs:  # an accessibility mask: runs of missing windows over a quarter of every row (the handle's *_mr kernels)
        frac, run = 0.25, int(rng.choice([20, 60]))
        for r in range(d.N):
            pos = int(rng.geometric(frac / (run * (1 - frac)))) - 1
            while pos < L:
                n = 8 + int(rng.geometric(1.0 / run))
                data[r, pos : pos + n] = -1
                pos += n + int(rng.geometric(frac / (run * (1 - frac))))
    for r in np.nonzero((data == -1).all(axis=1))[0]:  # the kernel object rejects all-missing rows
        data[r, int(rng.integers(0, L))] = int(rng.integers(2))
    d.data = data
    d.per_chunk = bool(rng.integers(2)) and d.S > 1
    Sp = d.S if d.per_chunk else 1
    pop = _population(d.K, d.B * Sp, seed=100 + seed)  # per chunk: one valid model per (particle, chunk), all different
    d.pp = pn.PP(*(a.reshape(d.B, Sp, d.K) for a in pop))
    d.nrm = int(rng.choice([1, 2, 4]))
    per_seq = ((L + 7) // 8) * d.Kc * (8 if d.dbl else 4)  # bytes of checkpoint store per sequence (phk_api.hip)
    want = ["none", "particles", "chunks"][int(rng.integers(3))]
    if want == "particles" and d.B < 2:
        want = "chunks"
    if want == "chunks" and d.S < 2:
        want = "particles" if d.B >= 2 else "none"
    d.ws, d.ws_limit, d.slab = want, None, (d.B, d.S)
    if want == "particles":  # slabs of whole particles
        nb = int(rng.integers(1, d.B))
        d.ws_limit, d.slab = per_seq * d.S * nb + int(rng.integers(0, per_seq)), (nb, d.S)
    elif want == "chunks":  # one particle, fewer chunks than the call has
        ns = int(rng.integers(1, d.S))
        d.ws_limit, d.slab = per_seq * ns + int(rng.integers(0, per_seq)), (1, ns)
    d.raw = seed % 3 == 0  # the call goes through the raw HipEngine method with device tensors
    d.lens = None
    if kind == "viterbi":
        mode = int(rng.integers(3))
        if mode and L - d.W >= 2:
            d.lens = rng.integers(d.W + 1, L + 1, size=d.N)
            if mode == 2:
                d.lens[d.inds[0]] = d.W + 1
                if d.S > 1 and d.inds[1] != d.inds[0]:
                    d.lens[d.inds[1]] = L
        return d
    Rs, Rsw, Rsg = plan_lists(d.Kc, d.dbl)
    form = int(rng.integers(3)) if L < 1025 else int(rng.choice([0, 1, 2, 2]))
    t16 = bool(rng.integers(2))
    ok16 = [r for r in Rs if d.Kc // r <= 4]
    dense16 = d.Kc == 16 and not d.dbl and rng.random() < 0.6
    if dense16 and rng.integers(2):
        d.nrm = 4  # the one-state-per-lane forward kernel with its dense steps
    d.plan = None
    if form:
        T = 16 if t16 and [r for r in (Rsw if form == 1 else Rsg) if r in ok16] else 8  # (T = 16: <= 4 states per lane)
        pick = lambda rs: int(rng.choice([r for r in rs if T == 8 or r in ok16]))  # noqa: E731
        Rf = 16 if dense16 else pick(Rs)
        if form == 1:
            d.plan = ("serial", pick(Rsw), T, Rf, 0)
        else:
            d.plan = ("segmented", pick(Rsg), T, Rf, int(rng.choice(Rs)))
    n = L - d.W
    bins = [1, 2, 7, 8, 16, 100, 512, 513, 1000, max(n, 1), n + 5]
    d.bin = int(bins[rng.integers(len(bins))])
    if d.plan is not None and d.plan[0] == "segmented" and L > UNIT_SITES:
        e = int(rng.integers(5))
        if e == 0:
            d.bin = int(rng.choice([513, 1000, max(n, 1), n + 5]))
        elif e in (1, 2):  # a bin whose last site is the first (e = 1) / the last (e = 2) site of a unit
            d.bin = int(rng.choice([2, 7, 8, 16, 100, 513]))
            d.W = (1 - d.bin) % UNIT_SITES if e == 1 else (UNIT_SITES - d.bin) % UNIT_SITES
    vform = int(rng.integers(3))
    d.values = None
    if vform == 1:
        d.values = np.linspace(0.1, 5.0, d.K) * float(rng.uniform(0.5, 2.0))
    elif vform == 2:
        d.values = np.cumsum(rng.uniform(0.05, 1.0, size=(d.B, d.K)), axis=1) * rng.uniform(0.2, 5.0, size=(d.B, 1))
    d.marginals = bool(rng.integers(2)) or d.values is None
    return (d, rng) if with_rng else d


@functools.lru_cache(maxsize=None)
def draw(seed, kind):
    """Deterministic, CPU only.  A float32 posterior draw on which float32 itself (``fb32``) keeps less than F32_REDRAW_BAR / 5
    is redrawn as float64, as the likelihood fuzz does with 50 % hets."""
    assert kind in ("posterior", "viterbi")
    d = _draw(seed, kind, False)
    if kind == "posterior" and not d.dbl and 5.0 * float(oracle_posterior(d)["E"].max(initial=0.0)) > F32_REDRAW_BAR:
        d = _draw(seed, kind, True)
        d.redrawn = True
    return d


# ------------------------------------------------------------------------------------------------- float32 emulations
def fb32(pp, data, W=0):
    """``posterior_oracle.forward_backward`` with every array and every operation in float32 (the dense model is built in
    float64 and rounded once).  -> (gamma [L - W, K] float32, ll)"""
    f = np.float32
    A = pn.dense_from_pp(pp).astype(f)
    e = [np.asarray(pp.emis0, float).astype(f), np.asarray(pp.emis1, float).astype(f), np.ones(A.shape[0], f)]
    codes = vo._codes(data)
    L, K = len(codes), A.shape[0]
    alpha = np.empty((L, K), f)
    c = np.empty(L, f)
    a = np.asarray(pp.pi, float).astype(f)
    for t in range(L):
        a = (a @ A) * e[codes[t]]
        c[t] = a.sum(dtype=f)
        a = a / c[t]
        alpha[t] = a
    gamma = np.empty((L, K), f)
    b = np.ones(K, f)
    for t in range(L - 1, -1, -1):
        g = alpha[t] * b
        tot = g.sum(dtype=f)
        # (a model with massless states, tests/massless_fuzz.py: where float32 has lost the live states' share of b the products
        # are exact zeros, and the figure is 0 -- an error of 1, the draw is run as float64 -- not 0 / 0)
        gamma[t] = g / tot if tot > 0 else f(0)
        b = A @ (e[codes[t]] * b)
        b = b / b.sum(dtype=f)
    return gamma[W:], float(np.log(c[W:].astype(float)).sum())


def structured_viterbi(pp, data, real=np.float64):
    """The step the Viterbi kernels run, stated with loops: the folded model (b, d, v) <- emis0 .* (b, d, v) with emission rows
    (1, emis1 / emis0, 1 / emis0); per site delta'_j = e_j max(v_j max_{i<j} u_i delta_i, d_j delta_j, b_j max_{i>j} delta_i)
    from one exclusive prefix maximum and one exclusive suffix maximum, each with the lowest index that reaches it; linear
    domain, rescaled by the power of two of the maximum.  ``real``: the float type of every product and comparison; the
    folded model is formed in float64 and rounded to it once.  -> (path [n], logp)"""
    r = real
    e0, e1 = np.asarray(pp.emis0, float), np.asarray(pp.emis1, float)
    b, d, v = ([r(x) for x in np.asarray(x, float) * e0] for x in (pp.b, pp.d, pp.v))
    u = [r(x) for x in np.asarray(pp.u, float)]
    rows = [[r(1.0)] * len(e0), [r(x) for x in e1 / e0], [r(x) for x in 1.0 / e0]]
    K = len(e0)
    zero = r(0.0)
    delta = [r(x) for x in np.asarray(pp.pi, float)]
    E = 0
    back = []
    for ob in data:
        e = rows[2 if ob < 0 else min(int(ob), 1)]
        pre, pa = [zero] * K, [0] * K
        run, arg = zero, 0
        for j in range(K):
            pre[j], pa[j] = run, arg
            c = u[j] * delta[j]
            if c > run:
                run, arg = c, j
        suf, sa = [zero] * K, [K - 1] * K
        run, arg = zero, K - 1
        for j in range(K - 1, -1, -1):
            suf[j], sa[j] = run, arg
            if delta[j] >= run:
                run, arg = delta[j], j
        new, ptr = [zero] * K, [0] * K
        for j in range(K):
            best, a = v[j] * pre[j], pa[j]
            c = d[j] * delta[j]
            if c > best:
                best, a = c, j
            c = b[j] * suf[j]
            if c > best:
                best, a = c, sa[j]
            new[j], ptr[j] = best * e[j], a
        ex = math.frexp(max(new))[1]
        delta = [r(math.ldexp(float(x), -ex)) for x in new]
        E += ex
        back.append(ptr)
    z = max(range(K), key=lambda j: (delta[j], -j))
    logp = E * math.log(2.0) + math.log(float(delta[z]))
    path = np.empty(len(data), dtype=np.uint8)
    for t in range(len(data) - 1, -1, -1):
        path[t] = z
        z = back[t][z]
    return path, logp


def sv32(pp, data):
    return structured_viterbi(pp, data, np.float32)


# ------------------------------------------------------------------------------------------------- oracles of a draw
def _gamma_error(g, g_ref, values):
    """per-site error of one evaluation against the oracle: gamma, and the values-weighted mean scaled by max |values|"""
    if g_ref.size == 0:
        return 0.0
    err = float(np.abs(g - g_ref).max())
    if values is not None:
        err = max(err, float(np.abs(g @ values - g_ref @ values).max() / np.abs(values).max()))
    return err


def _values_of(d, b):
    if d.values is None:
        return None
    return d.values[b] if d.values.ndim == 2 else d.values


def oracle_posterior(d):
    """-> {"gamma": [B][S] float64 [L - W, K], "ll": [B, S], "E": [B, S] (float32 draws: the per-site error of fb32)}"""
    if getattr(d, "_oracle", None) is None:
        cache, G = {}, []
        LL, E = np.empty((d.B, d.S)), np.zeros((d.B, d.S))
        for b in range(d.B):
            G.append([])
            for s in range(d.S):
                key = d.block_id(b, s) + (int(d.inds[s]),)
                if key not in cache:
                    q, row = d.block(b, s), d.data[d.inds[s]]
                    g, ll = po.forward_backward(q, row, d.W)
                    e = 0.0 if d.dbl else _gamma_error(fb32(q, row, d.W)[0].astype(float), g, _values_of(d, b))
                    cache[key] = (g, ll, e)
                g, LL[b, s], E[b, s] = cache[key]
                G[b].append(g)
        d._oracle = {"gamma": G, "ll": LL, "E": E}
    return d._oracle


def oracle_viterbi(d, want_margin=True):
    """-> {"path": [B][S] uint8 [n - W], "logp": [B, S], "margin": [B, S]}, n the own length of every row"""
    if getattr(d, "_oracle", None) is None:
        cache, P = {}, []
        LP, M = np.empty((d.B, d.S)), np.empty((d.B, d.S))
        for b in range(d.B):
            P.append([])
            for s in range(d.S):
                n = d.row_len(s)
                key = d.block_id(b, s) + (int(d.inds[s]), n)
                if key not in cache:
                    cache[key] = vo.viterbi(d.block(b, s), d.data[d.inds[s], :n], d.W, want_margin=want_margin)
                p, LP[b, s], M[b, s] = cache[key]
                P[b].append(p)
        d._oracle = {"path": P, "logp": LP, "margin": M}
    return d._oracle


def posterior_candidate(d, gammas, ll):
    """what a call of draw ``d`` returns if its per-site posteriors are ``gammas`` [B][S]: binned, stacked, the outputs the
    draw asks for"""
    out = {"ll": np.array(ll, float), "mean": None, "marginals": None}
    if d.marginals:
        out["marginals"] = np.array([[po.bin_means(gammas[b][s], d.bin) for s in range(d.S)] for b in range(d.B)]).reshape(
            d.B, d.S, d.nbin, d.K)
    if d.values is not None:
        out["mean"] = np.array([[po.bin_means(gammas[b][s] @ _values_of(d, b), d.bin) for s in range(d.S)]
                                for b in range(d.B)]).reshape(d.B, d.S, d.nbin)
    return out


def viterbi_candidate(d, paths, logp):
    """... if its paths are ``paths`` [B][S] (each of its row's own length): padded with 255"""
    path = np.full((d.B, d.S, d.L - d.W), 255, dtype=np.uint8)
    for b in range(d.B):
        for s in range(d.S):
            path[b, s, : len(paths[b][s])] = paths[b][s]
    return {"logp": np.array(logp, float), "path": path}


# ------------------------------------------------------------------------------------------------- comparators
FAIL = float("inf")


def gamma_bars(d, oracle):
    """[B, S]: the bar of every sequence"""
    if d.dbl:
        return np.full((d.B, d.S), F64_GAMMA_BAR)
    return np.maximum(F32_GAMMA_BAR, 5.0 * oracle["E"])


def compare_posterior(oracle, cand, d):
    """-> (worst error / bar over everything compared, message, {"gamma": worst raw error}).  A ratio above 1 -- inf for a
    wrong shape, a non-finite or negative posterior, a padded state -- fails the draw."""
    nbin, tol = d.nbin, (1e-12 if d.dbl else 2e-6)  # (tol: test_identities)
    ll = np.asarray(cand["ll"], float)
    if ll.shape != (d.B, d.S):
        return FAIL, f"ll shape {ll.shape}", {}
    if (cand["marginals"] is None) != (not d.marginals) or (cand["mean"] is None) != (d.values is None):
        return FAIL, "outputs present do not match what was asked for", {}
    worst, msg, raw = 0.0, "ok", 0.0

    def hold(ratio, text):
        nonlocal worst, msg
        if not ratio <= worst:  # (NaN counts as a failure)
            worst, msg = (ratio if ratio == ratio else FAIL), text

    ll_ref = oracle["ll"]
    atol, rtol = (1e-10, 1e-10) if d.dbl else (max(2e-5, 1e-7 * d.L), 1e-5)
    r = np.abs(ll - ll_ref) / (atol + rtol * np.abs(ll_ref))
    hold(float(r.max()), f"ll {ll.ravel()[r.argmax()]!r} vs oracle {ll_ref.ravel()[r.argmax()]!r}")
    bars = gamma_bars(d, oracle)
    m = mu = None
    if d.marginals:
        m = np.asarray(cand["marginals"], float)
        if m.shape != (d.B, d.S, nbin, d.K):
            return FAIL, f"marginals shape {m.shape}, expected {(d.B, d.S, nbin, d.K)}", {}
        if not np.isfinite(m).all() or (m < 0).any():
            return FAIL, "marginals not finite or negative", {}
        if nbin:
            hold(float(np.abs(m.sum(-1) - 1).max() / (16 * tol)), "bin rows do not sum to 1")
    if d.values is not None:
        mu = np.asarray(cand["mean"], float)
        if mu.shape != (d.B, d.S, nbin):
            return FAIL, f"mean shape {mu.shape}, expected {(d.B, d.S, nbin)}", {}
        if not np.isfinite(mu).all():
            return FAIL, "mean not finite", {}
    vmax = None if d.values is None else float(np.abs(d.values).max())
    for b in range(d.B):
        for s in range(d.S):
            g = oracle["gamma"][b][s]
            err = 0.0
            if m is not None and nbin:
                err = float(np.abs(m[b, s] - po.bin_means(g, d.bin)).max())
            if mu is not None and nbin:
                err = max(err, float(np.abs(mu[b, s] - po.bin_means(g @ _values_of(d, b), d.bin)).max()) / vmax)
            raw = max(raw, err)
            hold(err / bars[b, s], f"gamma of (particle {b}, chunk {s}): error {err:.3e}, bar {bars[b, s]:.3e}")
    return worst, msg, {"gamma": raw}


def compare_viterbi(oracle, cand, d):
    """-> (worst ratio, message, {"deficit": worst, "n_seq": sequences, "n_deficit_only": float64 sequences below MIN_MARGIN,
    "n_diff": sites that differ})"""
    logp, path = np.asarray(cand["logp"], float), np.asarray(cand["path"])
    if logp.shape != (d.B, d.S) or path.shape != (d.B, d.S, d.L - d.W) or path.dtype != np.uint8:
        return FAIL, f"shapes {logp.shape} {path.shape} {path.dtype}", {}
    worst, msg = 0.0, "ok"
    info = {"deficit": 0.0, "n_seq": d.B * d.S, "n_deficit_only": 0, "n_diff": 0}

    def hold(ratio, text):
        nonlocal worst, msg
        if not ratio <= worst:
            worst, msg = (ratio if ratio == ratio else FAIL), text

    eps = EPS[d.dbl]
    for b in range(d.B):
        q = d.block(b, 0)
        A = None
        for s in range(d.S):
            if d.per_chunk or A is None:
                q = d.block(b, s)
                A = pn.dense_from_pp(q)
            n, where = d.row_len(s), f"(particle {b}, chunk {s})"
            z, ref = path[b, s, : n - d.W], oracle["path"][b][s]
            if not (path[b, s, n - d.W :] == 255).all():
                return FAIL, f"{where}: bytes past the row's own length {n} are not 255", info
            if int(z.max()) >= d.K:
                return FAIL, f"{where}: state {int(z.max())} in the path, K = {d.K}", info
            zi = z.astype(int)
            if not (A[zi[:-1], zi[1:]] > 0).all():
                return FAIL, f"{where}: the path takes a step with A = 0", info
            differ = z != ref
            n_diff = int(differ.sum()) + (d.W if differ[0] else 0)
            info["n_diff"] += int(differ.sum())
            deficit = vo.deficit(q, d.data[d.inds[s], :n], ref, z, d.W) if n_diff else 0.0
            info["deficit"] = max(info["deficit"], deficit)
            if deficit < 0.0:
                return FAIL, f"{where}: deficit {deficit:.3e} < 0: a path above the oracle's", info
            if n_diff:
                bound = VITERBI_DEFICIT_ROUNDINGS * eps * n_diff
                hold(deficit / bound, f"{where}: deficit {deficit:.3e} over {n_diff} differing sites, bound {bound:.3e}")
            if d.dbl:
                if oracle["margin"][b, s] >= MIN_MARGIN:
                    if n_diff:
                        return FAIL, f"{where}: {int(differ.sum())} sites differ from the oracle's path, margin {oracle['margin'][b, s]:.2e}", info
                else:
                    info["n_deficit_only"] += 1
            ref_lp = oracle["logp"][b, s]
            bar = 1e-11 * abs(ref_lp) if d.dbl else F32_LOGP_BAR * abs(ref_lp) + max(2e-5, 1e-7 * d.L)
            hold(abs(logp[b, s] - ref_lp) / bar, f"{where}: logp {logp[b, s]!r} vs oracle {ref_lp!r}")
    return worst, msg, info


# ------------------------------------------------------------------------------------------------- a seeded fault
def viterbi_with_flipped_pointer(pp, data, W, t_flip):
    """The oracle's recursion with ONE backpointer wrong: at site ``t_flip``, for the state the best path is in there, the
    second-best predecessor.  -> path [n - W]"""
    logA, le, lpi = vo._log_tables(pp)
    codes = vo._codes(data)
    n, K = len(codes), len(lpi)
    back = np.empty((n, K), dtype=np.int64)
    second = None
    ld = lpi.copy()
    for t in range(n):
        cand = ld[:, None] + logA
        back[t] = cand.argmax(0)
        if t == t_flip:
            second = np.argsort(-cand, axis=0, kind="stable")[1]
        ld = cand[back[t], np.arange(K)] + le[codes[t]]
    z = int(ld.argmax())
    path = np.empty(n, dtype=np.uint8)
    for t in range(n - 1, -1, -1):
        path[t] = z
        z = int(second[z]) if t == t_flip else int(back[t, z])
    return path[W:]
