"""Seeded random draws of models with MASSLESS states -- pi = b = v = 0 on a set of dead states: nothing starts there and nothing
arrives there, the convention of tests/test_sweep_valu.py -- for the likelihood and gradient kernels (the fields and plans of
tests/model_fuzz.py) and for posterior and Viterbi decoding (the draws of tests/decode_fuzz.py with their models overwritten).
Test infrastructure only, CPU only, numpy only.  Used by tests/test_massless_fuzz.py.

Every other seeded fuzz draws strictly positive models; the kernels treat exact zeros as legal input, and a model with dead
states reaches code no ordinary draw reaches: scan totals and carries that are exact zeros, substochastic dense operators, a beta
scan whose mass sits in states the forward vector never enters, seed normalisation at unit edges, log 0 in Viterbi.

Patterns (``live_states``), per particle or, for a per-chunk block, per chunk:
    one-low      one live state: state 0; K / 4 where the draw is "mild" (see below)
    one-mid      one live state: K / 3
    two-far      two live states far apart: K / 4 and 2 K / 3 (K = 4: 1 and 2)
    lower-half   states [0, K / 2) dead (a mild draw at K = 4: state 0 alone; with state 1 dead as well the oracle's gradient is 3e12
                 after 2,600 sites)
    upper-half   states [K / 2, K) dead
    both-ends    (0, 1, K - 2, K - 1) dead; (0, K - 1) below K = 8
    two-middle   (K / 2 - 1, K / 2) dead
    every-second the odd states dead
    per-chunk    a different one of the above in every chunk of one particle

The float64 oracle alone decides what a valid draw is (tests/test_massless_fuzz.py asserts it for every default seed and forced
case): finite ll and gradient, the W = 0 gradient included; for a float32 kernel object a largest |d ll / d theta| of at most
GRAD_CAP_F32 = 1e12 (a product of two such figures still fits float32); every row of positive probability.  The draws are BUILT to
satisfy this, none is rejected: the dead entries of b, v and pi have one-sided derivatives that grow like
(d_j emis0_j / d_k emis0_k)^n for a dead state j that would explain the row better than the live state k, so a lone live state at
the top of the time axis has a gradient of 1e35 after 65 sites and none at all (NaN from the oracle itself) after 2,600.  Hence:
hets are few (1 ... 3 per row, at block and unit edges), the lone live states are the ones listed, and a "mild" draw -- one for a
float32 kernel object -- moves the low live state from 0 (6e17 after 65 sites at K = 16) to K / 4.
"""

from __future__ import annotations

import functools

import numpy as np

import decode_fuzz as df
import model_fuzz as mf
from oracle import psmc_numpy as pn

PATTERNS = ("one-low", "one-mid", "two-far", "lower-half", "upper-half", "both-ends", "two-middle", "every-second")
RICH_PATTERNS = ("one-top", "lower-half", "two-middle", "every-second")  # decoder draws at >= 10 % hets
FORMS = ("mixed", "all-massless", "batch-of-one", "wave33", "wave40")  # how the massless particles sit in the batch
LS = [8, 65, 513, 1040, 2600]  # the last two give a segmented plan several units
GRAD_CAP_F32 = 1e12
DEAD_ROWS = (0, 3, 6)  # b, v, pi of a block [7, K]
DECODE_SEED_BASE = 7_000  # the decoder draws are decode_fuzz._draw(DECODE_SEED_BASE + seed, kind, ...): seeds of their own
EDGES = (0, 7, 8, 15, 16, 63, 64, 511, 512, 513, 1023, 1024, 1535, 1536, 2047, 2048)


# ------------------------------------------------------------------------------------------------- patterns
def live_states(pattern, K, mild=False):
    """-> sorted list of the states that keep their mass"""
    if pattern == "one-low":
        live = {K // 4 if mild else 0}
    elif pattern == "one-mid":
        live = {K // 3}
    elif pattern == "one-top":  # (not among PATTERNS: outside every cap, see NEIGHBOUR_CASES)
        live = {K - 1}
    elif pattern == "two-far":
        live = {max(1, K // 4), (2 * K) // 3}
    elif pattern == "lower-half":
        live = set(range(1 if (mild and K == 4) else K // 2, K))
    elif pattern == "upper-half":
        live = set(range(K // 2))
    elif pattern == "both-ends":
        live = set(range(K)) - ({0, 1, K - 2, K - 1} if K >= 8 else {0, K - 1})
    elif pattern == "two-middle":
        live = set(range(K)) - {K // 2 - 1, K // 2}
    elif pattern == "every-second":
        live = set(range(0, K, 2))
    else:
        raise ValueError(pattern)
    assert live and live < set(range(K)), (pattern, K)
    return sorted(live)


def dead_mask(pattern, K, mild=False):
    m = np.ones(K, bool)
    m[live_states(pattern, K, mild)] = False
    return m


def kill(block, dead):
    """block [7, K] with pi = b = v = 0 on ``dead`` [K] bool (a copy)"""
    out = np.array(block, float)
    for r in DEAD_ROWS:
        out[r, dead] = 0.0
    return out


# ------------------------------------------------------------------------------------------------- data
def _rows(rng, N, L, W):
    """rows the live states can explain: 1 ... 3 hets per row (one at 8 sites), at block and unit edges and at the warm-up
    boundary; runs of missing sites, in some draws 1 % scattered missing sites as well"""
    data = np.zeros((N, L), np.int8)
    edges = sorted({e for e in EDGES + (L - 1, L // 2, W - 1, W) if 0 <= e < L})
    for r in range(N):
        for e in rng.choice(edges, size=min(len(edges), 1 if L <= 8 else int(rng.integers(1, 4))), replace=False):
            data[r, int(e)] = 1
    if rng.integers(2):
        data[rng.random((N, L)) < 0.01] = -1
    mf._missing_runs(rng, data, (1, 2), 50)
    for r in np.nonzero((data == -1).all(axis=1))[0]:
        data[r, int(rng.integers(0, L))] = 0
    return data


# ------------------------------------------------------------------------------------------------- likelihood draws
def _finish(d, rng, plan=None):
    d.het = float((d.data == 1).mean())
    n8 = (d.L // 8) * 8
    d.has_missing_runs = bool(n8 and (d.data[:, :n8].reshape(d.N, n8 // 8, 8) == -1).all(-1).any())
    d.mask_runs = None
    d.plan = mf._draw_plan(rng, d) if plan is None else plan
    if d.plan[0] == "plan":
        d.tags.add("plan:segmented" if d.plan[1] else "plan:serial")
    else:
        d.tags.add(f"plan:{d.plan[0]}")
    d.tags.add("family:dense16" if "dense16" in d.tags else "family:lanes")
    d.tags.add("f64" if d.dbl else "f32")
    for tag, on in (("dlog", d.dlog), ("f32-block", d.f32_block), ("per-chunk", d.per_chunk), ("mask-runs", d.mask_runs is not None),
                    ("beside-ordinary", any(b in d.odd and ((b > 0 and b - 1 not in d.odd) or (b + 1 < d.B and b + 1 not in d.odd))
                                            for b in range(d.B)))):
        if on:
            d.tags.add(tag)
    return d


def _fill(d, rng, massless, pattern_of):
    """P [B, Sp, 7, K]: ordinary particles of model_fuzz (every emis0 >= 0.5), the ones in ``massless`` with dead states"""
    Sp = d.S if d.per_chunk else 1
    d.mild = not d.dbl
    P = np.empty((d.B, Sp, 7, d.K))
    d.dead = np.zeros((d.B, Sp, d.K), bool)
    d.patterns = {}
    d.P_parent = np.empty_like(P)  # the blocks before any state was killed (for the seeded faults)
    for b in range(d.B):
        base = mf.ordinary(rng, d.K)
        for s in range(Sp):
            P[b, s] = d.P_parent[b, s] = base if not d.per_chunk else mf.ordinary(rng, d.K)
            if b in massless:
                pat = pattern_of(b, s)
                d.patterns[(b, s)] = pat
                d.dead[b, s] = dead_mask(pat, d.K, d.mild)
                P[b, s] = kill(P[b, s], d.dead[b, s])
                d.tags.add(f"pat:{pat}")
        if b in massless and Sp > 1 and len({d.patterns[(b, s)] for s in range(Sp)}) > 1:
            d.tags.add("pat:per-chunk")
    d.P = P
    d.odd = sorted(massless)


def _draw(seed):
    rng = np.random.default_rng([41_000, seed])
    form, j = FORMS[seed % 5], seed // 5
    d = mf.Draw(seed=seed, regime=form, tags={"massless", form}, form=None, odd=[])
    d.K = mf.KS[seed % 7]
    d.dbl = bool(rng.integers(2))
    d.L = L = LS[(j + seed % 5) % 5]
    d.B, d.S = int(rng.integers(2, 14)), int(rng.integers(1, 6))
    if form == "batch-of-one":
        d.B = 1
    elif form in ("wave33", "wave40"):  # one / two observation rows in a wave of the K = 16 kernels, as tests/test_sweep_valu.py
        d.B, d.S, d.K = (33 if form == "wave33" else 40), int(rng.integers(2, 4)), 16
        d.dbl = j % 4 == 3
    d.per_chunk = bool(rng.integers(2)) and d.S > 1
    d.N = d.S + int(rng.integers(0, 3))
    d.inds = rng.integers(0, d.N, size=d.S)
    d.W = int(rng.integers(0, L + 1)) if rng.integers(2) else 0
    d.nrm = int(rng.choice([1, 2, 4]))
    d.dlog = bool(rng.integers(2))
    d.f32_block = bool(rng.random() < 0.3)
    if form == "mixed":  # every second particle: each massless one has an ordinary neighbour in its wave
        massless = set(range(1, d.B, 2))
    elif form in ("all-massless", "batch-of-one"):
        massless = set(range(d.B))
    else:  # the residues of test_sweep_valu.py, and two more
        massless = {b for b in range(d.B) if b % 8 in (1, 2, 3, 5, 6)}
    shift = int(rng.integers(len(PATTERNS)))
    _fill(d, rng, massless, lambda b, s: PATTERNS[(shift + b + (s if d.per_chunk else 0)) % len(PATTERNS)])
    d.data = _rows(rng, d.N, L, d.W)
    return _finish(d, rng)


@functools.lru_cache(maxsize=None)
def draw(seed):
    """Deterministic, CPU only."""
    return _draw(int(seed))


# The forced cases: the plan of the note in tests/test_sweep_valu.py (K = 16 float32, one state per lane in the forward kernel and
# the beta scan, the two-lane segment sweep) and its serial and hybrid siblings, a one-live-state particle among ordinary ones.
# name -> (B, S, L, plan of model_fuzz._draw_plan, patterns by particle)
def _note_plan(kind, B):
    return {"segmented": ("plan", 1, 2, 8, 16, 16), "serial": ("plan", 0, 2, 8, 1, 0), "hybrid": ("hybrid", f"2:1:{B}:2:16")}[kind]


FORCED = {
    "one_live_segmented_3x2_1040": (3, 2, 1040, "segmented", {1: "one-mid"}),  # the smallest shape of the note with two units
    "one_live_serial_3x2_1040": (3, 2, 1040, "serial", {1: "one-mid"}),
    "one_live_hybrid_3x2_1040": (3, 2, 1040, "hybrid", {1: "one-mid"}),
    "one_live_segmented_3x2_2600": (3, 2, 2600, "segmented", {1: "one-mid"}),
    "one_low_segmented_3x2_1040": (3, 2, 1040, "segmented", {1: "one-low"}),
    "patterns_segmented_33x2_2600": (33, 2, 2600, "segmented", None),
    "patterns_hybrid_40x2_1040": (40, 2, 1040, "hybrid", None),
}


# One particle whose only live state is the LAST (2,600 sites: the first as well), among ordinary ones.  Its own gradient is 1e113
# after 1,040 sites in the float64 oracle -- float32 returns inf or NaN for it, and nothing here judges it -- but what the call
# returns for its ORDINARY neighbours must not depend on it.  On the parent of the commit that added this file every sequence
# that shared a 16-lane row with it came back NaN (ll of the gradient call and every gradient row), under the serial plan with the
# underflow flag clear: profiles/massless_fuzz.txt.
NEIGHBOUR_CASES = {
    "top_live_segmented_3x2_1040": (3, 2, 1040, "segmented", {1: "one-top"}),
    "top_live_serial_3x2_1040": (3, 2, 1040, "serial", {1: "one-top"}),
    "top_live_hybrid_3x2_1040": (3, 2, 1040, "hybrid", {1: "one-top"}),
    "top_live_segmented_33x2_2600": (33, 2, 2600, "segmented", {1: "one-top", 20: "one-top"}),
    "top_live_lanes8_5x2_1040": (5, 2, 1040, ("plan", 1, 8, 8, 8, 8), {2: "one-top"}),  # eight lanes per sequence: the other scan
}


@functools.lru_cache(maxsize=None)
def forced(name):
    B, S, L, kind, pats = (FORCED if name in FORCED else NEIGHBOUR_CASES)[name]
    rng = np.random.default_rng([42_000, sorted(list(FORCED) + list(NEIGHBOUR_CASES)).index(name)])
    d = mf.Draw(seed=name, regime="forced", tags={"massless", "forced", "dense16"}, form=None, odd=[])
    d.K, d.dbl, d.B, d.S, d.L, d.N, d.W = 16, False, B, S, L, S, 0
    d.per_chunk, d.nrm, d.dlog, d.f32_block = False, 4, False, False
    d.inds = np.arange(S)
    if pats is None:
        pats = {b: PATTERNS[(b // 8 + b % 8) % len(PATTERNS)] for b in range(B) if b % 8 in (1, 2, 3, 5, 6)}
    _fill(d, rng, set(pats), lambda b, s: pats[b])
    d.data = _rows(rng, d.N, L, 0)
    return _finish(d, rng, plan=kind if isinstance(kind, tuple) else _note_plan(kind, B))


def oracle_conditions(d):
    """-> list of the reference-alone conditions the draw misses (empty: valid)"""
    o = mf.oracle(d)
    bad = []
    if not np.isfinite(o["ll"]).all():
        bad.append("ll not finite (a row without probability under some particle)")
    if not np.isfinite(o["g"]).all():
        bad.append("gradient not finite")
    if o["g_full"] is not None and not np.isfinite(o["g_full"]).all():
        bad.append("W = 0 gradient not finite")
    gmax = max(float(np.abs(o["g"]).max()), float(np.abs(o["g_full"]).max()) if o["g_full"] is not None else 0.0)
    if not d.dbl and not gmax <= GRAD_CAP_F32:
        bad.append(f"largest |d ll / d theta| {gmax:.3g} above the float32 cap")
    if not (d.P_model[..., 4, :] >= 0.5).all():
        bad.append("an emis0 below 0.5")
    return bad


# ------------------------------------------------------------------------------------------------- decoder draws
def _decode_massless(d, seed):
    """overwrite d.pp: every particle massless on every fourth seed and in a batch of one, else every second one.  The rows stay as
    drawn, so at 10 % and 50 % hets the patterns are those of RICH_PATTERNS: under a pattern that keeps only low states a dead
    upper state explains such a row better by a factor per het, and the float64 oracle itself ends in 0 / 0 (one-low at K = 16,
    2,600 sites; upper-half at K = 32, 512 sites)."""
    pp = [np.array(a, float) for a in d.pp]  # b, d, u, v, emis0, emis1, pi: [B, Sp, K]
    B, Sp, K = pp[0].shape
    d.dead = np.zeros((B, Sp, K), bool)
    d.patterns = {}
    for b in range(B):
        if B >= 2 and seed % 4 and b % 2 == 0:
            continue
        for s in range(Sp):
            pats = PATTERNS if d.het < 0.1 else RICH_PATTERNS
            pat = pats[(seed + b + s) % len(pats)]
            d.patterns[(b, s)] = pat
            d.dead[b, s] = dead_mask(pat, K)
    for r in DEAD_ROWS:
        pp[r][d.dead] = 0.0
    d.pp = pn.PP(*pp)
    d._oracle = None
    d.massless_seed = seed
    return d


@functools.lru_cache(maxsize=None)
def decode_draw(seed, kind):
    """decode_fuzz's draw with massless models, everything else as drawn; the project's redraw rule for float32 posterior draws"""
    assert kind in ("posterior", "viterbi")
    d = _decode_massless(df._draw(DECODE_SEED_BASE + seed, kind, False), seed)
    if kind == "posterior" and not d.dbl and 5.0 * float(df.oracle_posterior(d)["E"].max(initial=0.0)) > df.F32_REDRAW_BAR:
        d = _decode_massless(df._draw(DECODE_SEED_BASE + seed, kind, True), seed)
        d.redrawn = True
    return d


def dead_of(d, b, s):
    return d.dead[b, s if d.per_chunk else 0]
