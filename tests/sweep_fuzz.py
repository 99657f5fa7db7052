"""Seeded random draws for the three sweeps that ride on ``phk_posterior``'s dispatch (``phk_transitions``, ``phk_predictive``,
``phk_tracts``), float32 emulations of their float64 dense oracles, and the comparators that hold a candidate output against
the oracle.  Test infrastructure only, CPU only; used by tests/test_sweep_fuzz.py (the GPU tests and the CPU self-tests share
the comparators).

A draw is the posterior draw of tests/decode_fuzz.py (K, float type, B x S, inds with repeats, L, W up to L, het / missing
rates, missing runs, broadcast or per-chunk blocks, rescale interval, both slab branches, raw or API call, plan, bin) from a
random stream of its own, plus: ``lens`` by data row (none, ragged, ragged with a row at W + 1 and one at L); transitions:
which outputs are asked for; tracts: the weight form and whether every particle has a row of its own.

Bars.  Nothing here is measured on the kernels.  The float64 references are transition_oracle.pair_posteriors,
predictive_oracle.loo and tract_oracle.dense; ``trans32`` / ``loo32`` / ``tract32`` are the same dense statements with every
array and every operation in float32 (the dense model is built in float64 and rounded once).
* Bin means and probabilities (``arrivals``, ``prob``), absolute error, per sequence.  float64: the project's flat bar
  (transition_bars / tract_bars).  float32: max(project float32 bar, 5 x E), E the emulation's error on that sequence against
  the oracle -- per site (bin 1) for arrivals; at the draw's own bin and weights AND at bin 1 for prob, whichever is larger: one
  float32 evaluation of one bin can cancel by chance (the argument of decode_fuzz.py).
* Bin sums (``changes``, ``het_observed``, ``het_missing``, ``score``), per bin; ``changes`` and ``score`` as
  |x - ref| / max(1, |ref|).  The rounding error of a sum grows at most linearly in its terms and the project's bars were
  measured at bins of at most 100 sites.  float64: project bar x max(1, own sites in the bin / 100).  float32:
  max(project float32 bar, 5 x the sum over the bin's own sites of the emulation's per-site absolute error).
* A float32 draw whose largest 5 x E exceeds decode_fuzz.F32_REDRAW_BAR (sums: x max(1, own sites / 100)) is redrawn as float64.
* ``ll``: as decode_fuzz.compare_posterior judges it.
"""

from __future__ import annotations

import functools

import numpy as np

import decode_fuzz as df
import predictive_bars
import predictive_oracle as lo
import tract_bars
import tract_oracle as qo
import transition_bars
import transition_oracle as to
import viterbi_oracle as vo
from oracle import psmc_numpy as pn

KINDS = ("transitions", "predictive", "tracts")
WFORMS = ("prefix", "interior", "single", "ones", "frac_high", "frac_zeros")
FAIL = df.FAIL
BIN_SITES = 100  # the largest bin the project's bars of the bin sums were measured at


# ------------------------------------------------------------------------------------------------- the draw
def _weights(rng, form, rows, K):
    """[rows, K] in [0, 1]; rows > 1: rows that differ between particles (but for all ones)"""
    m = np.zeros((rows, K))
    if form == "prefix":
        c = rng.integers(1, K + 1, size=rows)
        if rows > 1 and (c == c[0]).all():
            c[0] = c[0] % K + 1
        for r in range(rows):
            m[r, : c[r]] = 1.0
    elif form == "interior":
        for r in range(rows):
            a = int(rng.integers(0, K - 1))
            m[r, a : int(rng.integers(a + 1, K + 1))] = 1.0
        if rows > 1 and (m == m[0]).all():
            m[0] = 1.0 - m[0] if m[0].sum() < K else np.eye(K)[0]
    elif form == "single":
        k = rng.integers(0, K, size=rows)
        if rows > 1 and (k == k[0]).all():
            k[0] = (k[0] + 1) % K
        m[np.arange(rows), k] = 1.0
    elif form == "ones":
        m[:] = 1.0
    elif form == "frac_high":
        m = 1.0 - 0.1 * rng.random((rows, K))  # (0.9, 1]
    else:  # [0, 1] with some exact zeros, one per row at least
        m = rng.random((rows, K))
        m[rng.random((rows, K)) < 0.3] = 0.0
        m[np.arange(rows), rng.integers(0, K, size=rows)] = 0.0
    return m


def lens_and_long_bin(d, rng):
    """the sweep draws' long-bin rule and their three lens modes, drawn from ``rng`` after the posterior draw's fields"""
    if d.plan is not None and d.plan[0] == "segmented" and d.L - d.W > df.UNIT_SITES and d.n_units >= 2 and rng.integers(4) == 0:
        d.bin = int(rng.choice([513, 1000]))  # a bin longer than a unit, more often than the posterior draw has it
    mode = int(rng.integers(3))
    d.lens_mode = 0
    if mode and d.L - d.W >= 2:  # (always None at W = L; the Viterbi draw's three modes)
        d.lens_mode = mode
        d.lens = rng.integers(d.W + 1, d.L + 1, size=d.N)
        if mode == 2:
            d.lens[d.inds[0]] = d.W + 1
            if d.S > 1 and d.inds[1] != d.inds[0]:
                d.lens[d.inds[1]] = d.L


def _draw(seed, kind, force_dbl):
    d, rng = df._draw(seed, kind, force_dbl, with_rng=True)
    lens_and_long_bin(d, rng)
    if kind == "transitions":
        d.arrivals = bool(rng.integers(3))
        flip = bool(rng.integers(2))
        d.changes = not (d.raw and d.arrivals and flip)  # (changes can be switched off through the raw method only)
    elif kind == "tracts":
        d.wform = WFORMS[int(rng.integers(len(WFORMS)))]
        d.w_rows = bool(rng.integers(2)) and d.B > 1
        m = _weights(rng, d.wform, d.B if d.w_rows else 1, d.K)
        d.weights = m if d.w_rows else m[0]
    return d


def describe(d):
    s = (f"seed={d.seed} K={d.K} {'f64' if d.dbl else 'f32'}{'(redrawn)' if d.redrawn else ''} B={d.B} S={d.S} N={d.N} "
         f"inds={d.inds.tolist()} L={d.L} W={d.W} het={d.het} miss={d.miss} runs={int(d.runs)} {'chunk' if d.per_chunk else 'bcast'} "
         f"nrm={d.nrm} ws={d.ws} {'raw' if d.raw else 'api'} plan={d.plan} bin={d.bin} lens={None if d.lens is None else d.lens.tolist()}")
    if d.kind == "transitions":
        s += f" arrivals={int(d.arrivals)} changes={int(d.changes)}"
    if d.kind == "tracts":
        s += f" weights={d.wform}{'[B,K]' if d.w_rows else '[K]'}"
    return s


@functools.lru_cache(maxsize=None)
def draw(seed, kind):
    """Deterministic, CPU only.  A float32 draw on which the float32 emulation of the oracle itself keeps less than the redraw
    cap / 5 is redrawn as float64."""
    assert kind in KINDS
    d = _draw(seed, kind, False)
    if not d.dbl and oracle(d)["redraw"] > 1.0:
        d = _draw(seed, kind, True)
        d.redrawn = True
    return d


# ------------------------------------------------------------------------------------------------- float32 emulations
def _model32(pp):
    f = np.float32
    A = pn.dense_from_pp(pp).astype(f)
    e = [np.asarray(pp.emis0, float).astype(f), np.asarray(pp.emis1, float).astype(f), np.ones(A.shape[0], f)]
    pi = np.asarray(pp.pi, float).astype(f)
    return A, e, pi / pi.sum(dtype=f)


def trans32(pp, data, W=0):
    """``transition_oracle.pair_posteriors`` + ``arrivals_of`` in float32 -> arr [L - W, 3, K] float32"""
    f = np.float32
    A, e, a = _model32(pp)
    codes = vo._codes(data)
    L, K = len(codes), A.shape[0]
    before = np.empty((L, K), f)
    for t in range(L):
        before[t] = a
        a = (a @ A) * e[codes[t]]
        a = a / a.sum(dtype=f)
    out = np.empty((L, 3, K), f)
    b = np.ones(K, f)
    for t in range(L - 1, W - 1, -1):
        w = e[codes[t]] * b
        x = before[t][:, None] * A * w[None, :]
        x = x / x.sum(dtype=f)
        out[t, 0] = np.diagonal(x)
        out[t, 1] = np.triu(x, 1).sum(0, dtype=f)
        out[t, 2] = np.tril(x, -1).sum(0, dtype=f)
        b = A @ w
        b = b / b.sum(dtype=f)
    return out[W:]


def loo32(pp, data, W=0):
    """``predictive_oracle.loo`` in float32 -> (phet [L - W], score [L - W]) float32"""
    f = np.float32
    A, e, a = _model32(pp)
    codes = vo._codes(data)
    L, K = len(codes), A.shape[0]
    pred = np.empty((L, K), f)
    for t in range(L):
        pred[t] = a @ A
        a = pred[t] * e[codes[t]]
        a = a / a.sum(dtype=f)
    phet, score = np.zeros(L, f), np.zeros(L, f)
    b = np.ones(K, f)
    for t in range(L - 1, W - 1, -1):
        cav = pred[t] * b
        n = (cav @ e[0], cav @ e[1])
        tot = f(n[0] + n[1])
        phet[t] = n[1] / tot
        if codes[t] < 2:
            score[t] = np.log(f(n[codes[t]] / tot))
        b = A @ (e[codes[t]] * b)
        b = b / b.sum(dtype=f)
    return phet[W:], score[W:]


def tract32(pp, data, m, W, bins, length):
    """``tract_oracle.dense`` in float32 for one weight row m [K] and a tuple of bin sizes -> [tract [nbin] float32 per size]"""
    f = np.float32
    A, e, a0 = _model32(pp)
    codes = vo._codes(data)
    L, K = len(codes), A.shape[0]
    al = np.empty((L + 1, K), f)
    al[0] = a0
    for t in range(L):
        a = (al[t] @ A) * e[codes[t]]
        al[t + 1] = a / a.sum(dtype=f)
    m = np.asarray(m, float).astype(f)
    out = [np.zeros((L - W + bn - 1) // bn, f) for bn in bins]
    last = [{en: k for k, s, en in qo._bins(L, W, bn)} for bn in bins]
    first = [{s: k for k, s, en in qo._bins(L, W, bn)} for bn in bins]
    b = np.ones(K, f)
    q = np.zeros((len(bins), K), f)
    for t in range(L - 1, W - 1, -1):
        for g in range(len(bins)):
            if t in last[g]:
                q[g] = b
        et = e[codes[t]]
        q = ((m * et if t < length else et) * q) @ A.T
        b = A @ (et * b)
        z = b.sum(dtype=f)
        b, q = b / z, q / z
        if t < length:
            for g in range(len(bins)):
                if t in first[g]:
                    out[g][first[g][t]] = (q[g] @ al[t]) / (b @ al[t])
    return out


# ------------------------------------------------------------------------------------------------- oracles of a draw
def own_counts(d, n_own):
    """[nbin]: sites of every bin among the first ``n_own`` scored sites (the row's own)"""
    k = np.arange(d.nbin)
    return np.clip(np.minimum((k + 1) * d.bin, min(n_own, d.L - d.W)) - k * d.bin, 0, None)


def bin_sums(x, d, n_own):
    """x [L - W, ...] per scored site -> [nbin, ...]: sums over every bin's own sites"""
    x = np.asarray(x, float)
    pad = np.zeros((d.nbin * d.bin,) + x.shape[1:])
    n = min(n_own, x.shape[0])
    pad[:n] = x[:n]
    return pad.reshape((d.nbin, d.bin) + x.shape[1:]).sum(1)


def weight_row(d, b):
    return d.weights[b] if d.w_rows else d.weights


def _sum_scale(d, n_own):
    """[nbin]: what a bar of a bin sum measured at bins of <= 100 sites is multiplied by"""
    return np.maximum(1.0, own_counts(d, n_own) / BIN_SITES)


def oracle(d):
    """-> {"ll": [B, S], "seq": [B][S] dict of the sequence's reference outputs, their bars' float32 terms and per-site
    arrays, "redraw": the largest 5 x E over its cap (float32 draws)}; computed once per (parameter block, data row, own
    length[, weight row]) and kept on the draw"""
    if getattr(d, "_oracle", None) is not None:
        return d._oracle
    site, seqs, out = {}, {}, []
    LL = np.empty((d.B, d.S))
    redraw = 0.0
    cap = df.F32_REDRAW_BAR
    for b in range(d.B):
        out.append([])
        for s in range(d.S):
            row, q, length = d.data[d.inds[s]], d.block(b, s), d.row_len(s)
            n_own = length - d.W
            key = d.block_id(b, s) + (int(d.inds[s]),)
            skey = key + (length,) + ((b,) if d.kind == "tracts" and d.w_rows else ())
            if skey not in seqs:
                o = {"n_own": n_own, "cnt": own_counts(d, n_own)}
                scale = _sum_scale(d, n_own)
                if d.kind == "transitions":
                    if key not in site:
                        xi, ll = to.pair_posteriors(q, row, d.W)
                        arr = to.arrivals_of(xi)
                        e_a = e_c = None
                        if not d.dbl:
                            a32 = trans32(q, row, d.W).astype(float)
                            e_a = np.abs(a32 - arr).max((1, 2), initial=0.0)
                            e_c = np.abs(a32[:, 1:].sum(-1) - arr[:, 1:].sum(-1))
                        site[key] = (arr, ll, e_a, e_c)
                    arr, ll, e_a, e_c = site[key]
                    A, C = to.reduce_bins(arr, d.W, d.bin, length)
                    o.update(arr=arr, ll=ll, arrivals=A, changes=C)
                    if not d.dbl:
                        o["E_arrivals"] = float(e_a[:n_own].max(initial=0.0))
                        o["E_changes"] = bin_sums(e_c, d, n_own)
                        if d.arrivals:
                            redraw = max(redraw, 5.0 * o["E_arrivals"] / cap)
                        if d.changes:
                            redraw = max(redraw, float((5.0 * o["E_changes"] / (cap * scale[:, None])).max(initial=0.0)))
                elif d.kind == "predictive":
                    if key not in site:
                        phet, score, ll = lo.loo(q, row, d.W)
                        e_p = e_s = None
                        if not d.dbl:
                            p32, s32 = loo32(q, row, d.W)
                            e_p, e_s = np.abs(p32.astype(float) - phet), np.abs(s32.astype(float) - score)
                        site[key] = (phet, score, ll, e_p, e_s)
                    phet, score, ll, e_p, e_s = site[key]
                    o.update(phet=phet, score=score, ll=ll, track=lo.reduce_bins(phet, score, row, d.W, d.bin, length))
                    if not d.dbl:
                        obs = row[d.W :] >= 0
                        o["E_track"] = np.stack([bin_sums(e_p * obs, d, n_own), bin_sums(e_p * ~obs, d, n_own), bin_sums(e_s, d, n_own)], -1)
                        redraw = max(redraw, float((5.0 * o["E_track"] / (cap * scale[:, None])).max(initial=0.0)))
                else:
                    m = weight_row(d, b)
                    if d.dbl:
                        prob, ll = qo.dense(q, row, m, d.W, d.bin, length)
                    else:
                        (prob, p1), ll = qo.dense(q, row, m, d.W, (d.bin, 1), length)
                        q32, q1 = tract32(q, row, m, d.W, (d.bin, 1), length)
                        o["E_prob"] = max(float(np.abs(q32 - prob).max(initial=0.0)), float(np.abs(q1 - p1).max(initial=0.0)))
                        redraw = max(redraw, 5.0 * o["E_prob"] / cap)
                    o.update(prob=prob, ll=ll)
                seqs[skey] = o
            out[b].append(seqs[skey])
            LL[b, s] = seqs[skey]["ll"]
    d._oracle = {"ll": LL, "seq": out, "redraw": redraw}
    return d._oracle


# ------------------------------------------------------------------------------------------------- candidates (CPU tests)
def _f(d):
    return "float64" if d.dbl else "float32"


def _lens_of(d, row_len):
    return [d.row_len(s) if row_len is None else int(row_len(s)) for s in range(d.S)]


def transitions_candidate(d, arrs, ll, row_len=None):
    """what a call of draw ``d`` returns if its per-site (stay, up, down) are ``arrs`` [B][S] and the rows' own lengths are
    ``row_len(s)`` (default: the draw's)"""
    n = _lens_of(d, row_len)
    red = [[to.reduce_bins(arrs[b][s], d.W, d.bin, n[s]) for s in range(d.S)] for b in range(d.B)]
    A = np.array([[r[0] for r in row] for row in red]).reshape(d.B, d.S, d.nbin, 3, d.K)
    C = np.array([[r[1] for r in row] for row in red]).reshape(d.B, d.S, d.nbin, 2)
    return {"ll": np.array(ll, float), "dtype": _f(d), "arrivals": A if d.arrivals else None, "changes": C if d.changes else None}


def predictive_candidate(d, phets, scores, ll, row_len=None):
    n = _lens_of(d, row_len)
    T = np.array([[lo.reduce_bins(phets[b][s], scores[b][s], d.data[d.inds[s]], d.W, d.bin, n[s]) for s in range(d.S)]
                  for b in range(d.B)]).reshape(d.B, d.S, d.nbin, 3)
    return {"ll": np.array(ll, float), "dtype": _f(d), "het_observed": T[..., 0], "het_missing": T[..., 1], "score": T[..., 2]}


def tracts_candidate(d, ll, row_len=None, weights=None, shift=0):
    """... from the dense oracle with the rows' own lengths ``row_len(s)``, the weight row ``weights(b)`` and the bins moved
    ``shift`` sites to the right"""
    n = _lens_of(d, row_len)
    P = np.zeros((d.B, d.S, d.nbin))
    for b in range(d.B):
        for s in range(d.S):
            m = weight_row(d, b) if weights is None else weights(b)
            p = qo.dense(d.block(b, s), d.data[d.inds[s]], m, d.W + shift, d.bin, n[s])[0]
            P[b, s, : len(p)] = p[: d.nbin]
    return {"ll": np.array(ll, float), "dtype": _f(d), "prob": P}


def oracle_candidate(d):
    """the oracle's own output in the form of a call's"""
    o = oracle(d)
    per = lambda name: [[o["seq"][b][s][name] for s in range(d.S)] for b in range(d.B)]  # noqa: E731
    if d.kind == "transitions":
        return transitions_candidate(d, per("arr"), o["ll"])
    if d.kind == "predictive":
        return predictive_candidate(d, per("phet"), per("score"), o["ll"])
    P = np.array(per("prob")).reshape(d.B, d.S, d.nbin)
    return {"ll": o["ll"].copy(), "dtype": _f(d), "prob": P}


# ------------------------------------------------------------------------------------------------- comparators
class _Judge:
    def __init__(self):
        self.worst, self.msg = 0.0, "ok"

    def hold(self, ratio, text):
        if not ratio <= self.worst:  # (NaN counts as a failure)
            self.worst, self.msg = (ratio if ratio == ratio else FAIL), text


def _hold_ll(j, d, ll, ll_ref):
    """ll as decode_fuzz.compare_posterior judges it"""
    atol, rtol = (1e-10, 1e-10) if d.dbl else (max(2e-5, 1e-7 * d.L), 1e-5)
    r = np.abs(ll - ll_ref) / (atol + rtol * np.abs(ll_ref))
    j.hold(float(r.max()), f"ll {ll.ravel()[r.argmax()]!r} vs oracle {ll_ref.ravel()[r.argmax()]!r}")


def _array(cand, name, shape, d):
    """-> (float64 array, None) or (None, message)"""
    x = cand[name]
    if x is None:
        return None, f"{name} is None"
    x = np.asarray(x, float)
    if x.shape != shape:
        return None, f"{name} shape {x.shape}, expected {shape}"
    if not np.isfinite(x).all():
        return None, f"{name} not finite"
    return x, None


def compare(oracle, cand, d):
    """-> (worst error / bar over everything compared, message, {name: worst raw figure}).  A ratio above 1 -- inf for a wrong
    shape or type, a missing or unasked-for output, a non-finite value, a broken exact property -- fails the draw."""
    ll = np.asarray(cand["ll"], float)
    if ll.shape != (d.B, d.S):
        return FAIL, f"ll shape {ll.shape}", {}
    if cand.get("dtype") != _f(d):
        return FAIL, f"outputs are {cand.get('dtype')}, the handle's type is {_f(d)}", {}
    j = _Judge()
    _hold_ll(j, d, ll, oracle["ll"])
    fail = {"transitions": _compare_transitions, "predictive": _compare_predictive, "tracts": _compare_tracts}[d.kind]
    raw = {}
    msg = fail(j, raw, oracle, cand, d)
    if msg is not None:
        return FAIL, msg, raw
    return j.worst, j.msg, raw


def _compare_transitions(j, raw, oracle, cand, d):
    nbin, tol = d.nbin, (1e-12 if d.dbl else 2e-6)
    if (cand["arrivals"] is None) != (not d.arrivals) or (cand["changes"] is None) != (not d.changes):
        return "outputs present do not match what was asked for"
    a = c = None
    if d.arrivals:
        a, msg = _array(cand, "arrivals", (d.B, d.S, nbin, 3, d.K), d)
        if msg:
            return msg
    if d.changes:
        c, msg = _array(cand, "changes", (d.B, d.S, nbin, 2), d)
        if msg:
            return msg
    raw["arrivals"] = raw["changes"] = 0.0
    for b in range(d.B):
        for s in range(d.S):
            o, where = oracle["seq"][b][s], f"(particle {b}, chunk {s})"
            empty = o["cnt"] == 0
            if a is not None and nbin:
                if a[b, s][empty].any():
                    return f"{where}: arrivals of a bin without a site of the row's own are not 0"
                err = float(np.abs(a[b, s] - o["arrivals"]).max())
                bar = transition_bars.F64_ARRIVALS_BAR if d.dbl else max(transition_bars.F32_ARRIVALS_BAR, 5.0 * o["E_arrivals"])
                raw["arrivals"] = max(raw["arrivals"], err)
                j.hold(err / bar, f"arrivals of {where}: error {err:.3e}, bar {bar:.3e}")
                if not empty.all():
                    j.hold(float(np.abs(a[b, s][~empty].sum((-1, -2)) - 1).max() / (16 * tol)), f"{where}: stay + up + down does not sum to 1")
            if c is not None and nbin:
                if c[b, s][empty].any():
                    return f"{where}: changes of a bin without a site of the row's own are not 0"
                err = np.abs(c[b, s] - o["changes"]) / np.maximum(1.0, np.abs(o["changes"]))
                if d.dbl:
                    bar = transition_bars.F64_CHANGES_BAR * _sum_scale(d, o["n_own"])[:, None]
                else:
                    bar = np.maximum(transition_bars.F32_CHANGES_BAR, 5.0 * o["E_changes"])
                raw["changes"] = max(raw["changes"], float(err.max()))
                k = np.unravel_index((err / bar).argmax(), err.shape)
                j.hold(float((err / bar).max()), f"changes of {where}, bin {k[0]}: error {err[k]:.3e}, bar {np.broadcast_to(bar, err.shape)[k]:.3e}")
    return None


def _compare_predictive(j, raw, oracle, cand, d):
    nbin = d.nbin
    x = []
    for name in ("het_observed", "het_missing", "score"):
        v, msg = _array(cand, name, (d.B, d.S, nbin), d)
        if msg:
            return msg
        x.append(v)
    x = np.stack(x, -1)  # [B, S, nbin, 3]
    raw["het"] = raw["score"] = 0.0
    if not nbin:
        return None
    if d.bin == 1 and ((x[..., 0] != 0) & (x[..., 1] != 0)).any():
        return "het_observed and het_missing are both non-zero at one site"
    f64 = np.array([predictive_bars.F64_HET_BAR, predictive_bars.F64_HET_BAR, predictive_bars.F64_SCORE_BAR])
    f32 = np.array([predictive_bars.F32_HET_BAR, predictive_bars.F32_HET_BAR, predictive_bars.F32_SCORE_BAR])
    for b in range(d.B):
        for s in range(d.S):
            o, where = oracle["seq"][b][s], f"(particle {b}, chunk {s})"
            if x[b, s][o["cnt"] == 0].any():
                return f"{where}: a bin without a site of the row's own is not 0"
            ref = o["track"]
            err = np.abs(x[b, s] - ref)
            err[:, 2] /= np.maximum(1.0, np.abs(ref[:, 2]))
            bar = f64 * _sum_scale(d, o["n_own"])[:, None] if d.dbl else np.maximum(f32, 5.0 * o["E_track"])
            raw["het"], raw["score"] = max(raw["het"], float(err[:, :2].max())), max(raw["score"], float(err[:, 2].max()))
            k = np.unravel_index((err / bar).argmax(), err.shape)
            j.hold(float((err / bar).max()), f"{('het_observed', 'het_missing', 'score')[k[1]]} of {where}, bin {k[0]}: error {err[k]:.3e}, bar {bar[k]:.3e}")
    return None


def _compare_tracts(j, raw, oracle, cand, d):
    p, msg = _array(cand, "prob", (d.B, d.S, d.nbin), d)
    if msg:
        return msg
    raw["prob"] = 0.0
    if not d.nbin:
        return None
    if (p < 0).any() or (p > 1).any():
        return "prob outside [0, 1]"
    for b in range(d.B):
        for s in range(d.S):
            o, where = oracle["seq"][b][s], f"(particle {b}, chunk {s})"
            empty = o["cnt"] == 0
            if p[b, s][empty].any():
                return f"{where}: a bin without a site of the row's own is not 0"
            if d.wform == "ones" and (p[b, s][~empty] != 1.0).any():
                return f"{where}: all-ones weights and a prob that is not exactly 1"
            err = float(np.abs(p[b, s] - o["prob"]).max())
            bar = tract_bars.F64_TRACT_BAR if d.dbl else max(tract_bars.F32_TRACT_BAR, 5.0 * o["E_prob"])
            raw["prob"] = max(raw["prob"], err)
            j.hold(err / bar, f"prob of {where}: error {err:.3e}, bar {bar:.3e}")
    return None
