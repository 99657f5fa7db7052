"""Seeded random draws for the pair counts (``phk_pair_counts``), a float32 emulation of their float64 dense oracle, and the
comparator that holds a candidate output against the oracle.  Test infrastructure only, CPU only; used by
tests/test_pair_fuzz.py (the GPU tests and the CPU self-tests share the comparator).

A draw is the posterior draw of tests/decode_fuzz.py from a random stream of its own (stream 6), then the sweep draws' ``lens``
modes (tests/sweep_fuzz.lens_and_long_bin), then the fields drawn here: W = 0 moved onto a unit's first or last site under a
segmented plan with more than one unit, and the workspace limit.  ``bin``, ``values`` and ``marginals`` of the posterior draw are
ignored: pair counts run at bin 1.

Workspace limit.  ``slab_for`` counts, per sequence, the checkpoint store and the float64 partials of the plan with the most
units: ``bytes_per_seq``.  The limit is recomputed from it after W is final, so that the pair-count call is cut into the slab
the posterior draw wanted -- (nb, S) or (1, ns), at least two slabs; a gradient call under the same limit counts checkpoints only
and gets a larger slab (``grad_slab``).

Bars.  Nothing here is measured on the kernels.  The reference is the dense float64 pair posterior of
``transition_oracle.pair_posteriors`` summed over the row's own scored sites (``pair_count_oracle.pair_counts``; here streamed,
xi_t is never kept); metric per entry |c - C| / max(1, C), the project's.  scale = max(1, own scored sites / 700): an entry is a
sum over the sites, its rounding error grows at most linearly in them, and the project's bars were measured on 700-site rows.
* float64: max(F64_COUNTS_BAR x scale, 5 x the sequence's loop-form floor), the floor being the distance of
  ``pair_count_oracle.loop_form`` (the kernel's sums in float64) from the dense oracle.
* float32, per entry: max(F32_COUNTS_BAR x scale, 5 x E[i, j] / max(1, C[i, j])), E[i, j] the sum over the own scored sites of
  |xi32_t[i, j] - xi_t[i, j]|, xi32 the same dense statement with every array and operation in float32 (``pairs32``): it bounds
  what float32 does to the entry with no cancellation between the sites.
* A float32 draw whose largest 5 x E / max(1, C) exceeds decode_fuzz.F32_REDRAW_BAR x scale is redrawn as float64.
* ``ll``: as sweep_fuzz._hold_ll.
"""

from __future__ import annotations

import functools

import numpy as np

import decode_fuzz as df
import pair_count_bars as bars
import pair_count_oracle as pco
import sweep_fuzz as sf
import transition_oracle as to
import viterbi_oracle as vo
from oracle import psmc_numpy as pn

KIND = "pairs"
FAIL = df.FAIL
BAR_SITES = 700  # the row length the project's bars were measured at
FLUSH_SITES = 64  # float32 sums go into the float64 partial this often (launch_pairs.hip)
LIFTED = 1 << 40  # a workspace limit no draw reaches


# ------------------------------------------------------------------------------------------------- the draw
def units(d, T, W=None):
    """``Draw.n_units`` with T passed in (phk_api.hip, n_units)"""
    W = d.W if W is None else W
    G = df.UNIT_SITES // T
    nblk = (d.L + T - 1) // T
    segW = ((W - 1) // T) // G if W > 0 else 0
    return (nblk + G - 1) // G - segW


def ckpt_bytes(d):
    return ((d.L + 7) // 8) * d.Kc * (8 if d.dbl else 4)


def bytes_per_seq(d):
    """what slab_for counts per sequence of a pair-count call: checkpoints + the partials of the plan with the most units"""
    return ckpt_bytes(d) + max(1, units(d, 8), units(d, 16)) * d.Kc * d.Kc * 8


def slab_under(limit, per_seq, B, S):
    """slab_for's rule -> (particles, chunks) per launch"""
    max_seq = max(1, limit // max(per_seq, 1))
    if B * S <= max_seq:
        return (B, S)
    return (max_seq // S, S) if max_seq >= S else (1, max_seq)


def row_tiles(d):
    """launches of the sweep per call of pairs_tn: one per tile of origin rows (launch_pairs.hip, pairs_rt)"""
    if d.dbl:
        return d.Kc // 4
    return 1 if d.Kc <= 16 else d.Kc // 8


def matrix_path(d):
    return d.Kc == 16 and not d.dbl


def seg(d):
    return d.plan is not None and d.plan[0] == "segmented"


def unit_own_sites(d):
    """own scored sites of every (sequence, unit) of the call under the draw's plan (no forced plan: one serial unit)"""
    edges = [(0, d.L)]
    if seg(d):
        T = d.plan[2]
        first = ((d.W - 1) // T) // (df.UNIT_SITES // T) if d.W > 0 else 0
        edges = [(0 if u == first else u * df.UNIT_SITES, min((u + 1) * df.UNIT_SITES, d.L)) for u in range(first, first + units(d, T))]
    return [max(0, min(hi, d.row_len(s)) - max(lo, d.W)) for s in range(d.S) for lo, hi in edges]


def _draw(seed, force_dbl):
    d, rng = df._draw(seed, KIND, force_dbl, with_rng=True)
    sf.lens_and_long_bin(d, rng)
    d.bin, d.values, d.marginals = 1, None, True  # (ignored: pair counts run at bin 1)
    # The shared fields put W on a unit's edge in none of the default seeds (four of them have a segmented plan and more than
    # one unit; W is 0 in two, inside a unit in two).  W = 0 is what the fixed grid of tests/test_pair_counts.py runs: under a
    # segmented plan with more than one unit it becomes a unit's first site (the unit left of it then owns no site) or the last
    # site of the unit before (which owns that one site), stratified by the seed as the row length is; lens follow W.
    e = (seed // 16) % 2
    if seg(d) and d.L > df.UNIT_SITES and d.W == 0:
        u = int(rng.integers(1, (d.L - 1) // df.UNIT_SITES + 1))
        d.W = u * df.UNIT_SITES - e  # e = 0: the first site of unit u, e = 1: the last site of unit u - 1
        if d.lens is not None:
            d.lens = np.maximum(d.lens, d.W + 1 + rng.integers(0, d.L - d.W, size=d.N))
            if d.lens_mode == 2:
                d.lens[d.inds[0]] = d.W + 1
                if d.S > 1 and d.inds[1] != d.inds[0]:
                    d.lens[d.inds[1]] = d.L
    # the workspace limit, by slab_for's rule for this sweep
    per = bytes_per_seq(d)
    d.ws_limit, d.grad_slab = None, (d.B, d.S)
    if d.ws == "particles":
        d.ws_limit = per * d.S * d.slab[0] + int(rng.integers(0, per))
    elif d.ws == "chunks":
        d.ws_limit = per * d.slab[1] + int(rng.integers(0, per))
    if d.ws_limit is not None:
        assert slab_under(d.ws_limit, per, d.B, d.S) == d.slab and d.slab != (d.B, d.S)
        d.grad_slab = slab_under(d.ws_limit, ckpt_bytes(d), d.B, d.S)
    d.raw = seed % 3 == 0
    return d


def describe(d):
    return (f"seed={d.seed} K={d.K} {'f64' if d.dbl else 'f32'}{'(redrawn)' if d.redrawn else ''} B={d.B} S={d.S} N={d.N} "
            f"inds={d.inds.tolist()} L={d.L} W={d.W} het={d.het} miss={d.miss} runs={int(d.runs)} {'chunk' if d.per_chunk else 'bcast'} "
            f"nrm={d.nrm} ws={d.ws} slab={d.slab} grad_slab={d.grad_slab} {'raw' if d.raw else 'api'} plan={d.plan} "
            f"tiles={row_tiles(d)} lens={None if d.lens is None else d.lens.tolist()}")


@functools.lru_cache(maxsize=None)
def draw(seed):
    """Deterministic, CPU only.  A float32 draw on which the float32 emulation of the oracle itself keeps less than the redraw
    cap / 5 is redrawn as float64."""
    d = _draw(seed, False)
    if not d.dbl and oracle(d)["redraw"] > 1.0:
        d = _draw(seed, True)
        d.redrawn = True
    return d


def manual_draw(K, dbl, data, inds, pp, W, lens=None, plan=None, nrm=4, seed=-1):
    """a draw with given fields (the fixed-shape GPU tests): one block per particle, pp [B, 1, K]; no slabs, through the API"""
    data = np.asarray(data, np.int8)
    d = df.Draw(seed=seed, kind=KIND, redrawn=False, K=K, Kc=min(k for k in df.COMPILED_K if k >= K), dbl=dbl, L=data.shape[1],
                B=pp.pi.shape[0], S=len(inds), N=data.shape[0], inds=np.asarray(inds), W=W, het=float("nan"), miss=float("nan"),
                runs=False, data=data, per_chunk=False, pp=pp, nrm=nrm, ws="none", ws_limit=None, raw=False, plan=plan, bin=1,
                lens=None if lens is None else np.asarray(lens), lens_mode=0, values=None, marginals=True)
    d.slab = d.grad_slab = (d.B, d.S)
    return d


# ------------------------------------------------------------------------------------------------- oracle and emulation
def pairs32(pp, data, W=0):
    """``sweep_fuzz.trans32`` that yields the whole float32 xi_t: ``transition_oracle.pair_posteriors`` with every array and
    operation in float32 (the dense model is built in float64 and rounded once).  Yields (t, xi32_t [K, K]) for
    t = L - 1 .. W."""
    f = np.float32
    A, e, a = sf._model32(pp)
    codes = vo._codes(data)
    L, K = len(codes), A.shape[0]
    before = np.empty((L, K), f)
    for t in range(L):
        before[t] = a
        a = (a @ A) * e[codes[t]]
        a = a / a.sum(dtype=f)
    b = np.ones(K, f)
    for t in range(L - 1, W - 1, -1):
        w = e[codes[t]] * b
        x = before[t][:, None] * A * w[None, :]
        yield t, x / x.sum(dtype=f)
        b = A @ w
        b = b / b.sum(dtype=f)


def _pairs64(pp, data, W=0):
    """``transition_oracle.pair_posteriors``, streamed: yields (t, xi_t [K, K]) for t = L - 1 .. W, then (-1, ll)"""
    A = pn.dense_from_pp(pp)
    e0, e1, pi = (np.asarray(x, float) for x in (pp.emis0, pp.emis1, pp.pi))
    data = np.asarray(data).astype(int)
    L, K = len(data), len(pi)
    before = np.empty((L, K))
    c = np.empty(L)
    a = pi / pi.sum()
    c0 = pi.sum()
    for t in range(L):
        before[t] = a
        a = (a @ A) * to._emis(e0, e1, data[t])
        c[t] = a.sum()
        a = a / c[t]
    b = np.ones(K)
    for t in range(L - 1, W - 1, -1):
        w = to._emis(e0, e1, data[t]) * b
        x = before[t][:, None] * A * w[None, :]
        yield t, x / x.sum()
        b = A @ w
        b = b / b.sum()
    if L:
        c[0] *= c0
    yield -1, float(np.log(c[W:]).sum())


def sequence_oracle(pp, data, W, length, dbl):
    """-> {"C": [K, K], "ll", "n_own", and "E" [K, K] + "C32" (float32 draws) or "floor" (float64 draws)} of one sequence"""
    K = len(np.asarray(pp.pi))
    C = np.zeros((K, K))
    ll = None
    gen32 = None if dbl else pairs32(pp, data, W)
    E, C32 = np.zeros((K, K)), np.zeros((K, K))
    for t, x in _pairs64(pp, data, W):
        if t < 0:
            ll = x
            break
        x32 = None if dbl else next(gen32)[1]
        if t < length:
            C += x
            if not dbl:
                x32 = x32.astype(float)
                C32 += x32
                E += np.abs(x32 - x)
    o = {"C": C, "ll": ll, "n_own": max(length - W, 0)}
    if dbl:
        o["floor"] = pco.error(pco.loop_form(pp, data, W, length), C)
    else:
        o.update(E=E, C32=C32)
    return o


def scale_of(n_own):
    return max(1.0, n_own / BAR_SITES)


def entry_bars(o, dbl):
    """[K, K] (float32) or a scalar (float64): the bar of every entry of one sequence, on |c - C| / max(1, C)"""
    s = scale_of(o["n_own"])
    if dbl:
        return max(bars.F64_COUNTS_BAR * s, 5.0 * o["floor"])
    return np.maximum(bars.F32_COUNTS_BAR * s, 5.0 * o["E"] / np.maximum(1.0, o["C"]))


def oracle(d, shared=None):
    """-> {"ll": [B, S], "seq": [B][S] sequence_oracle dicts, "redraw": the largest 5 x E / max(1, C) over its cap (float32
    draws)}; computed once per (parameter block, data row, own length) and kept on the draw.  ``shared``: a dict that keeps the
    sequences between draws which share blocks and rows (the caller's keys: (particle, data row, own length))."""
    if getattr(d, "_oracle", None) is not None:
        return d._oracle
    seqs, out = {} if shared is None else shared, []
    LL = np.empty((d.B, d.S))
    redraw = 0.0
    for b in range(d.B):
        out.append([])
        for s in range(d.S):
            length = d.row_len(s)
            key = d.block_id(b, s) + (int(d.inds[s]), length)
            if key not in seqs:
                seqs[key] = sequence_oracle(d.block(b, s), d.data[d.inds[s]], d.W, length, d.dbl)
            o = seqs[key]
            out[b].append(o)
            LL[b, s] = o["ll"]
            if not d.dbl:
                redraw = max(redraw, float((5.0 * o["E"] / np.maximum(1.0, o["C"])).max()) / (df.F32_REDRAW_BAR * scale_of(o["n_own"])))
    d._oracle = {"ll": LL, "seq": out, "redraw": redraw}
    return d._oracle


# ------------------------------------------------------------------------------------------------- candidates (CPU tests)
def oracle_candidate(d, name="C"):
    """the oracle's own output (``name`` = "C32": the float32 emulation's) in the form of a call's"""
    o = oracle(d)
    C = np.array([[o["seq"][b][s][name] for s in range(d.S)] for b in range(d.B)]).reshape(d.B, d.S, d.K, d.K)
    return {"ll": o["ll"].copy(), "dtype": "float64", "counts": C}


def pairs_candidate(d, row_len=None, W=None, sites=None, matrix=None):
    """What a call of draw ``d`` returns if the rows' own lengths are ``row_len(s)`` (default: the draw's), the warm-up is ``W``,
    its per-site pair posteriors are ``sites(xi [n, K, K])`` and its summed matrix is ``matrix(C, b, s)``; ll is the oracle's.
    xi is recomputed here, for this draw only."""
    W = d.W if W is None else W
    cache = {}
    C = np.zeros((d.B, d.S, d.K, d.K))
    for b in range(d.B):
        for s in range(d.S):
            key = d.block_id(b, s) + (int(d.inds[s]),)
            if key not in cache:
                cache[key] = to.pair_posteriors(d.block(b, s), d.data[d.inds[s]], W)[0]
            xi = cache[key] if sites is None else sites(cache[key].copy())
            n = (d.row_len(s) if row_len is None else int(row_len(s))) - W
            c = xi[: max(n, 0)].sum(0)
            C[b, s] = c if matrix is None else matrix(c, b, s)
    return {"ll": oracle(d)["ll"].copy(), "dtype": "float64", "counts": C}


# ------------------------------------------------------------------------------------------------- the comparator
def compare(oracle, cand, d):
    """-> (worst error / bar over everything compared, message, {"counts": worst raw error, "total": worst |counts.sum() - own
    scored sites| (reported, not held)}).  A ratio above 1 -- inf for a wrong shape or type, a non-finite or negative entry, a
    non-zero output at W = L -- fails the draw."""
    ll = np.asarray(cand["ll"], float)
    if ll.shape != (d.B, d.S):
        return FAIL, f"ll shape {ll.shape}", {}
    if cand.get("dtype") != "float64":
        return FAIL, f"counts are {cand.get('dtype')}: float64 for either handle type", {}
    c = np.asarray(cand["counts"], float)
    if c.shape != (d.B, d.S, d.K, d.K):
        return FAIL, f"counts shape {c.shape}, expected {(d.B, d.S, d.K, d.K)}", {}
    if not np.isfinite(c).all() or (c < 0).any():
        return FAIL, "counts not finite or negative", {}
    if d.W == d.L and (c.any() or ll.any()):
        return FAIL, "W = L: counts and ll are not all 0", {}
    j = sf._Judge()
    sf._hold_ll(j, d, ll, oracle["ll"])
    raw = {"counts": 0.0, "total": 0.0}
    for b in range(d.B):
        for s in range(d.S):
            o, where = oracle["seq"][b][s], f"(particle {b}, chunk {s})"
            err = np.abs(c[b, s] - o["C"]) / np.maximum(1.0, o["C"])
            bar = np.broadcast_to(entry_bars(o, d.dbl), err.shape)
            raw["counts"] = max(raw["counts"], float(err.max()))
            raw["total"] = max(raw["total"], abs(float(c[b, s].sum()) - o["n_own"]))
            k = np.unravel_index((err / bar).argmax(), err.shape)
            j.hold(float((err / bar).max()), f"counts of {where}, entry {k}: error {err[k]:.3e}, bar {bar[k]:.3e}")
    return j.worst, j.msg, raw
