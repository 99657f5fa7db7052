"""Seeded random draws over MODEL space for the likelihood and gradient kernels (``phk_loglik``), in the style of
tests/decode_fuzz.py.  Test infrastructure only, CPU only, numpy only: models come from ``oracle.psmc_numpy`` (the reference's
own map particle -> demographic model -> HMM block, its 1e-20 clips included) and nothing from ``phlash_amd``.  Used by
tests/test_model_fuzz.py.

The kernels branch on the parameter block in five places ("Model-space fuzz"); every regime here is built to reach
one of them, mixed with ordinary particles inside one batch wherever the kernel decides per wave:

* wide        theta log-uniform over [1e-3, 10], a sigma in {0.3, 1, 2} population, data whose het rate follows theta.
* unfoldable  blocks with a float32 emis0 <= 2^-64 (theta x E[t_M] > 64 ln 2): (a) every block of the batch, (b) exactly one
              particle among >= 4 ordinary ones, (c) per-chunk blocks, one particle folding at chunk s and not at chunk s + 1.
* threshold   an ordinary block whose last state's emis0 is exactly 2^-63, 2^-64, 2^-65, or the float64 just above 2^-64
              (which float32 rounds to 2^-64), emis1 = 1 - emis0.
* steep       emis1 in every state one of {1e-3, 1e-6, 1e-11, 1e-20} in one or two particles, het runs of 4 ... 24 sites
              across block and segment edges in some rows.
* huge        2^-64 < min emis0 < 1e-6: the folded ratios exist and reach 2^64, on rows with runs of missing sites.

``draw(seed)`` is deterministic and returns plain numpy, so the decoding fuzz can reuse it.
"""

from __future__ import annotations

import functools
import math
import types

import numpy as np

import decode_fuzz as df
from oracle import psmc_numpy as pn

REGIMES = ("wide", "unfoldable", "threshold", "steep", "huge")
KS = [4, 8, 16, 16, 16, 32, 64]
LS = [8, 9, 64, 65, 513, 1025, 2600]
FOLD_MIN = 2.0 ** -64  # RATIO_MIN_EMIS0 of the kernels: a sequence folds iff every emis0, in the kernel's float type, is ABOVE it
ABOVE_FOLD_MIN = float(np.nextafter(FOLD_MIN, 1.0))  # float64 just above 2^-64; float32 rounds it to 2^-64
THRESHOLDS = (("2^-63", 2.0 ** -63), ("2^-64", FOLD_MIN), ("2^-65", 2.0 ** -65), ("2^-64+", ABOVE_FOLD_MIN))
STEEP_EMIS1 = (1e-3, 1e-6, 1e-11, 1e-20)
LN_FOLD = 64.0 * math.log(2.0)  # emis0 = exp(-theta E[t]) <= 2^-64  <=>  theta E[t] >= 44.36


# ------------------------------------------------------------------------------------------------- models
def pattern_of(K):
    """the pattern of ``_params`` in tests/test_hip_parity.py"""
    return f"{K - 2}*1+1*2" if K > 4 else f"{K}*1"


def model(rng, K, theta, sigma, t1=1e-4, pat=None, last_exponent=None):
    """One block [7, K] from the reference's map: from_dm(particle_to_dm(x0 + sigma N(0, 1))).  ``last_exponent`` = x: theta is
    rescaled so that the largest theta E[t_k] of this particle is x, i.e. its smallest emis0 is exp(-x) (before the 1e-20 clip)."""
    pat = pat or pattern_of(K)
    P = len(pn.parse_pattern(pat))
    x0 = pn.particle_from_linear(pat, t1, 15.0, np.ones(P), theta, theta)
    x = x0 + sigma * rng.normal(size=x0.shape)
    if last_exponent is not None:
        dm = pn.particle_to_dm(x, pat, theta)
        theta = theta * last_exponent / float((theta * pn.ect(dm.t, dm.c)).max())
    return pn.from_dm(pn.particle_to_dm(x, pat, theta)).stack()


def ordinary(rng, K):
    """a particle of ``_params``: the flat default model plus 0.3 sigma noise at theta = 1e-2"""
    return model(rng, K, 1e-2, 0.3)


def unfoldable(rng, K):
    return model(rng, K, 1.0, 0.3, last_exponent=float(rng.uniform(LN_FOLD + 0.2, 120.0)))


def huge(rng, K):
    return model(rng, K, 1.0, 0.3, last_exponent=float(rng.uniform(16.0, LN_FOLD - 2.0)))


def folds32(block):
    """[...] bool: the float32 kernels' (and ``phk_prefold``'s) test on blocks [..., 7, K]"""
    return (np.asarray(block)[..., 4, :].astype(np.float32) > np.float32(FOLD_MIN)).all(-1)


def folds64(block):
    """the float64 kernels' test"""
    return (np.asarray(block)[..., 4, :] > FOLD_MIN).all(-1)


# ------------------------------------------------------------------------------------------------- the draw
class Draw(types.SimpleNamespace):
    @property
    def P_model(self):
        """the block the kernels are handed, as float64: the float32-rounded block where it is handed over as float32 (then
        the exact model of the call), else the unrounded one"""
        return self.P.astype(np.float32).astype(np.float64) if self.f32_block else self.P

    def folds(self):
        """[B, Sp] bool: which blocks the kernels of this draw's float type fold"""
        return folds64(self.P_model) if self.dbl else folds32(self.P_model)

    def describe(self):
        return (f"seed={self.seed} {'+'.join(sorted(self.tags))} K={self.K} {'f64' if self.dbl else 'f32'} B={self.B} S={self.S} "
                f"N={self.N} inds={self.inds.tolist()} L={self.L} W={self.W} het={self.het:g} "
                f"{'chunk' if self.per_chunk else 'bcast'} nrm={self.nrm} plan={self.plan} mask_runs={self.mask_runs} "
                f"dlog={int(self.dlog)} block={'f32' if self.f32_block else 'f64'} odd={self.odd}")


def _missing_runs(rng, data, n_runs, max_len):
    max_len = max(1, min(max_len, data.shape[1] // 4))  # (short rows keep most of their sites)
    for r in range(data.shape[0]):
        for _ in range(int(rng.integers(n_runs[0], n_runs[1] + 1))):
            s0 = int(rng.integers(0, data.shape[1]))
            data[r, s0:s0 + int(rng.integers(1, max_len + 1))] = -1


def _draw_plan(rng, d):
    """As test_random_shapes_against_the_oracle (any K); for K = 16 float32 half the draws take the one-state-per-lane forms
    of test_dense_kernels_random_shapes.  -> ("variant", R, T) | ("plan", segmented, R, T, R_forward, R_scan) | ("tuner",) |
    ("hybrid", spec)"""
    K, dbl, n = d.K, d.dbl, d.B * d.S
    Rs, Rsw, Rsg = df.plan_lists(K, dbl)
    d.mask_runs = None
    if K == 16 and not dbl and rng.integers(2):
        d.tags.add("dense16")
        d.nrm = 4
        T = int(rng.choice([8, 16]))
        form = int(rng.integers(3))
        if d.has_missing_runs:
            d.mask_runs = [None, "1", "0"][int(rng.integers(3))]
        if form == 0:
            return ("variant", 16, T)
        if form == 1:
            return ("plan", 1, 4, T, 16, 16)
        if n >= 2:
            first = int(rng.integers(1, n))
            if d.S >= 2 and rng.integers(2):
                first = d.B * int(rng.integers(1, d.S))
            return ("hybrid", f"{int(rng.choice([2, 4, 16]))}:16:{first}:4:16")
        return ("plan", 1, 2, 8, 16, 16)
    mode = int(rng.integers(5))
    if mode == 0:
        R = int(rng.choice(Rsw))
        return ("variant", R, 16 if (K // R <= 4 and rng.integers(2)) else 8)
    if mode == 1:
        return ("plan", 1, int(rng.choice(Rsg)), 8, int(rng.choice(Rs)), int(rng.choice(Rs)))
    if mode == 2:
        return ("plan", 0, int(rng.choice(Rsw)), 8, int(rng.choice(Rs)), 0)
    if mode == 4 and n >= 2:
        return ("hybrid", f"{int(rng.choice(Rsw))}:{int(rng.choice(Rs))}:{int(rng.integers(1, n))}:{int(rng.choice(Rsg))}:{int(rng.choice(Rs))}")
    return ("tuner",)


def _draw(seed):
    rng = np.random.default_rng([31_000, seed])
    regime, j = REGIMES[seed % 5], seed // 5  # (j: the running number of the draw within its regime)
    d = Draw(seed=seed, regime=regime, tags={regime}, form=None, odd=[])
    d.K = K = KS[int(rng.integers(7))]
    d.dbl = bool(rng.integers(2))
    d.B, d.S = int(rng.integers(1, 14)), int(rng.integers(1, 6))
    d.L = L = LS[(3 * j + seed % 5) % 7]
    d.per_chunk = bool(rng.integers(2)) and d.S > 1
    if regime == "unfoldable":
        d.form = "abc"[j % 3]
        d.tags.add(f"unfoldable-{d.form}")
        if d.form == "b":
            d.B = int(rng.integers(5, 14))
            if (j // 3) % 4 != 3:  # the odd particle among others in the one-state-per-lane and scalar-code paths
                d.K, d.dbl = 16, False
                K = 16
        if d.form == "c":
            d.S, d.per_chunk = int(rng.integers(2, 6)), True
    if regime == "steep":
        d.B = int(rng.integers(2, 14))
    if regime == "threshold":  # mostly the float32 kernels: the predicate exists twice there (kernels and phk_prefold)
        d.dbl = (j // 4) % 4 == 3
    B, S = d.B, d.S
    Sp = S if d.per_chunk else 1
    d.N = S + int(rng.integers(0, 3))
    d.inds = rng.integers(0, d.N, size=S)
    d.W = int(rng.integers(0, L + 1)) if rng.integers(2) else 0
    d.nrm = int(rng.choice([1, 2, 4]))
    d.dlog = bool(rng.integers(2))
    d.f32_block = bool(rng.random() < 0.3)

    # ---- the parameter blocks [B, Sp, 7, K]
    P = np.empty((B, Sp, 7, K))
    d.het = float(rng.choice([0.005, 0.02, 0.05]))

    def fill(make):
        for b in range(B):
            for s in range(Sp):
                P[b, s] = make(b, s)

    if regime == "wide":
        theta = float(np.exp(rng.uniform(math.log(1e-3), math.log(10.0))))
        sigma, t1 = float(rng.choice([0.3, 1.0, 2.0])), float(rng.choice([1e-4, 1e-3]))
        pat = pattern_of(K) if rng.integers(2) else f"{K}*1"
        d.het = min(0.5, 3.0 * theta)
        d.wide = (theta, sigma, t1, pat)
        fill(lambda b, s: model(rng, K, theta, sigma, t1, pat))
    elif regime == "unfoldable":
        if d.form == "a":
            fill(lambda b, s: unfoldable(rng, K))
        elif d.form == "b":
            d.odd = [int(rng.integers(B))]
            fill(lambda b, s: unfoldable(rng, K) if b == d.odd[0] else ordinary(rng, K))
        else:
            d.odd, s0 = [int(rng.integers(B))], int(rng.integers(S - 1))
            d.flip_chunk = s0  # particle odd[0]: chunk s0 folds, chunk s0 + 1 does not
            fold_kind = huge if rng.integers(2) else ordinary
            fill(lambda b, s: unfoldable(rng, K) if (b == d.odd[0] and s == s0 + 1) else
                 (fold_kind(rng, K) if (b == d.odd[0] and s == s0) else ordinary(rng, K)))
    elif regime == "threshold":
        name, e0 = THRESHOLDS[j % 4]
        d.tags.add(f"emis0={name}")
        d.threshold = e0
        d.odd = sorted(rng.choice(B, size=int(rng.integers(1, min(B, 2) + 1)), replace=False).tolist()) if rng.integers(2) else list(range(B))
        fill(lambda b, s: ordinary(rng, K))
        for b in d.odd:
            P[b, :, 4, K - 1] = e0
            P[b, :, 5, K - 1] = 1.0 - e0
    elif regime == "steep":
        d.emis1 = STEEP_EMIS1[j % 4]
        d.tags.add(f"emis1={d.emis1:g}")
        d.odd = sorted(rng.choice(B, size=min(int(rng.integers(1, 3)), B - 1), replace=False).tolist())  # (B >= 2: waves are mixed)
        fill(lambda b, s: ordinary(rng, K))
        for b in d.odd:
            P[b, :, 5, :] = d.emis1
            P[b, :, 4, :] = 1.0 - d.emis1
        d.het = 0.01
    else:  # huge
        d.odd = list(range(B)) if rng.integers(2) else sorted(rng.choice(B, size=min(int(rng.integers(1, 3)), B), replace=False).tolist())
        fill(lambda b, s: huge(rng, K) if b in d.odd else ordinary(rng, K))
    d.P = P

    # ---- the data rows
    data = (rng.random((d.N, L)) < d.het).astype(np.int8)
    if rng.integers(2):
        data[rng.random((d.N, L)) < 0.05] = -1
    if regime == "huge":  # runs of missing sites in every row: 1 / emis0 in a lane at every one of them
        _missing_runs(rng, data, (2, 3), 80)
        n = max(4, min(L // 2, int(rng.integers(8, 81))))  # ... and one run of at least four in a row the call uses
        s0 = int(rng.integers(0, L - n + 1))
        data[int(d.inds[int(rng.integers(S))]), s0:s0 + n] = -1
    else:
        _missing_runs(rng, data, (1, 2), 50)
    if regime == "steep":  # het runs of 4 ... 24 sites across block (8), segment (512) and warm-up edges, in some rows only
        rows = [r for r in range(d.N) if rng.integers(2)]
        sure = int(d.inds[int(rng.integers(S))])  # a row the call uses gets one run that covers a whole block of eight
        edges = [e for e in (8, 16, 64, 512, 1024, 2048, d.W, L // 2) if 0 < e < L]
        for r in rows:
            for _ in range(int(rng.integers(1, 4))):
                n = int(rng.integers(4, 25))
                s0 = max(0, int(rng.choice(edges)) - int(rng.integers(0, n + 1))) if edges else 0
                data[r, s0:s0 + n] = 1
        if L >= 24:
            e = int(rng.choice([x for x in edges if x + 16 <= L] or [8]))
            s0 = max(0, e - int(rng.integers(0, 9)))
            data[sure, s0:s0 + 16 + int(rng.integers(0, 9))] = 1
        else:
            data[sure, 0:8] = 1
        d.steep_row = sure
    for r in np.nonzero((data == -1).all(axis=1))[0]:  # the kernel object rejects all-missing rows
        data[r, int(rng.integers(0, L))] = 0
    d.data = data
    n8 = (L // 8) * 8
    d.has_missing_runs = bool(n8 and (data[:, :n8].reshape(d.N, n8 // 8, 8) == -1).all(-1).any())
    d.plan = _draw_plan(rng, d)

    # ---- tags: what the block really is, by the predicate of the kernels that will run it
    f = d.folds()
    d.tags.add("foldable" if f.all() else "has-unfoldable")
    if not f.all() and f.any():
        d.tags.add("mixed-fold")
    if d.odd and len(d.odd) < B:
        d.tags.add("mixed")
    if d.dlog:
        d.tags.add("dlog")
    if d.f32_block:
        d.tags.add("f32-block")
    if d.per_chunk:
        d.tags.add("per-chunk")
    if d.mask_runs is not None:
        d.tags.add("mask-runs")
    return d


@functools.lru_cache(maxsize=None)
def draw(seed):
    """Deterministic, CPU only."""
    return _draw(int(seed))


# ------------------------------------------------------------------------------------------------- oracle-side figures
def block_mass_exponents(block, row, T=8):
    """log2 of what the oracle's forward recursion (dense form, psmc_numpy) loses over each aligned block of T sites of ``row``
    under ``block`` [7, K] -> [ceil(L / T)]"""
    pp = pn.PP(*block)
    A = pn.dense_from_pp(pp)
    alpha = np.array(pp.pi, float)
    out = np.zeros((len(row) + T - 1) // T)
    for t, ob in enumerate(np.asarray(row)):
        alpha = (alpha @ A) * pn.emission_row(pp, int(ob))
        c = alpha.sum()
        alpha = alpha / c
        out[t // T] += math.log2(c)
    return out


def oracle(d):
    """-> {"ll": [B, S], "g": [B, S, 7, K] d ll / d theta, "g_full": the W = 0 gradient or None}: ``cport.batch`` on the model the
    call is handed, computed once per draw"""
    if getattr(d, "_oracle", None) is None:
        from oracle import cport

        ll, g = cport.batch(d.P_model, d.data, d.inds, d.W)
        g_full = cport.batch(d.P_model, d.data, d.inds, 0)[1] if d.W > 0 else None
        d._oracle = {"ll": ll, "g": g, "g_full": g_full}
    return d._oracle
