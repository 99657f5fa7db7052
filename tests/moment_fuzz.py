"""Seeded random draws for the bin moments (``phk_bin_moments``), a float32 emulation of their float64 dense oracle, and the
comparator that holds a candidate output against the oracle.  Test infrastructure only, CPU only; used by
tests/test_moment_fuzz.py (the GPU tests and the CPU self-tests share the comparator).

A draw is the posterior draw of tests/decode_fuzz.py from a random stream of its own (stream 7), then the sweep draws' long-bin
rule and ``lens`` modes (tests/sweep_fuzz.lens_and_long_bin), then the fields drawn here: a segmented plan in place of a forced
serial one on some rows of more than two units, W = 0 moved onto a unit's first or last site under a segmented plan with more
than one unit, a bin longer than two units, the value form (stratified by the seed), whether every particle has a value row of
its own, for a call through ``PSMCKernel.bin_moments`` the map a + c v of the row into arbitrary units, and a bin of a few sites
in place of every other bin of one.  The
moment sweep carries no workspace of its own, so the posterior draw's workspace limit and slab hold as they are (asserted with
pair_fuzz.slab_under on the checkpoint bytes).  ``values`` and ``marginals`` of the posterior draw are ignored.

Raw and API calls.  A raw draw (seed % 3 == 0) gives ``HipEngine.bin_moments`` the row in [-1, 1].  Every other draw goes through
``PSMCKernel.bin_moments`` with a_b + c_b v_b (c_b log-uniform over 1e-3 .. 1e4, |a_b| = 0.1 .. 5 times c_b, so |a_b| runs over
1e-4 .. 5e4); ``centre`` recomputes the centre, the scale and the row the kernel runs on in numpy float64 from the draw's own pi
(per-chunk blocks: the sum of the chunks' pi rows), and the oracle runs on that row.  |a_b| / c_b stays below 5 so that an ulp
of the centre, which the host sums in another order than numpy does, moves a 100-site m1 by a tenth of the float64 bar at most.

Bars.  Nothing here is measured on the kernels.  The reference is ``moment_oracle.dense``; metric per bin, for m1 and m2
separately, |x - ref| / max(1, |ref|), the project's.  scale = max(1, the bin's own sites / 100): the project's bars were measured
at bins of at most 100 sites and the rounding error of a sum grows at most linearly in its terms.
* float64: max(F64_MOMENT_BAR x scale, 5 x the sequence's structured floor), the floor being the distance of
  ``moment_oracle.structured`` (the kernel's form in float64 loops) from the dense oracle on that sequence, per moment.
* float32, per bin: max(max(F32_MOMENT_BAR.values()) x scale, 5 x E).  The flat term is the same for every K: the per-K spread of
  moment_bars.F32_MEASURED comes from one cancelling 100-site sum on that grid's inputs, and random signed and alternating rows
  cancel at every K.  E is the error of ``moments32`` (the dense oracle with every array and operation in float32) on that bin
  at the draw's bin size and, for m1, the sum over the bin's own sites of its bin-1 m1 error (in the bin's units) if that is
  larger: one float32 evaluation of a bin can cancel by chance.
* A float32 draw whose largest 5 x E exceeds decode_fuzz.F32_REDRAW_BAR x scale is redrawn as float64.
* ``mean`` and ``var`` of an API draw: what the m1 and m2 bars allow after the map (tests/test_bin_moments.band_case), with
  d = bar1 max(1, |m1|): |d mean| <= s d, |d var| <= s^2 (bar2 max(1, m2) + 2 |m1| d + d^2); plus the float64 rounding of the map
  itself, (K + 8) eps (|s m1| + max |values| n) resp. 4 eps s^2 (m2 + m1^2) -- the centre is a K-term sum.
* ``ll``: as sweep_fuzz._hold_ll.
"""

from __future__ import annotations

import functools

import numpy as np

import decode_fuzz as df
import moment_bars as bars
import moment_oracle as mo
import pair_fuzz as pf
import sweep_fuzz as sf
import viterbi_oracle as vo

KIND = "moments"
FAIL = df.FAIL
FORMS = ("signed", "monotone", "indicator", "single", "alternating", "constant", "zeros")
BIN_SITES = sf.BIN_SITES  # the largest bin the project's bars were measured at
F32_FLAT_BAR = max(bars.F32_MOMENT_BAR.values())
LIFTED = pf.LIFTED
EPS64 = df.EPS[True]


# ------------------------------------------------------------------------------------------------- the draw
def _value_rows(rng, form, rows, K):
    """[rows, K] in [-1, 1]; rows > 1: rows that differ between particles (but for zeros)"""
    k = np.arange(K)
    m = np.zeros((rows, K))
    if form == "signed":
        m = rng.uniform(-1.0, 1.0, (rows, K))
    elif form == "monotone":  # (the centred rows of tests/test_bin_moments.grid_values)
        mid = (K - 1) / 2
        m = np.stack([(k - mid - r) / (mid + r) for r in range(rows)])
    elif form == "indicator":
        for r in range(rows):
            a = int(rng.integers(0, K - 1))
            m[r, a : int(rng.integers(a + 1, K + 1))] = 1.0
        if rows > 1 and (m == m[0]).all():
            m[0] = 1.0 - m[0] if m[0].sum() < K else np.eye(K)[0]
    elif form == "single":
        j = rng.integers(0, K, size=rows)
        sign = rng.choice([-1.0, 1.0], size=rows)
        if rows > 1 and (j == j[0]).all() and (sign == sign[0]).all():
            j[0] = (j[0] + 1) % K
        m[np.arange(rows), j] = sign
    elif form == "alternating":  # +1, -1, ..: the sign and the size change with the particle
        m = np.stack([(-1.0) ** (k + r) * (1.0 if r < 2 else 0.5) for r in range(rows)])
    elif form == "constant":
        c = rng.uniform(-1.0, 1.0, size=rows)
        c[np.abs(c) < 0.05] = 0.5
        if rows > 1 and len(set(c.tolist())) < rows:
            c = c[0] * (1.0 - 0.1 * np.arange(rows))
        m[:] = c[:, None]
    return m


def seg(d):
    return pf.seg(d)


def _draw(seed, force_dbl):
    d, rng = df._draw(seed, KIND, force_dbl, with_rng=True)
    sf.lens_and_long_bin(d, rng)
    d.values, d.marginals = None, True  # (ignored)
    # no workspace of the sweep's own: the posterior draw's limit cuts this call into the slab that draw wanted
    if d.ws_limit is not None:
        assert pf.slab_under(d.ws_limit, pf.ckpt_bytes(d), d.B, d.S) == d.slab and d.slab != (d.B, d.S)
    # The shared fields give no row of more than two units a segmented plan within the default seeds: on such a row every other
    # forced serial plan becomes a segmented one (the serial sweep's lanes per sequence are valid for a segment sweep too)
    if d.plan is not None and d.plan[0] == "serial" and d.L > 2 * df.UNIT_SITES and (seed // 16) % 2:
        d.plan = ("segmented",) + d.plan[1:4] + (int(rng.choice(df.plan_lists(d.Kc, d.dbl)[0])),)
    # W = 0 under a segmented plan with more than one unit: a unit's first site (the unit left of it owns nothing) or the last
    # site of the unit before (which owns that one site), as pair_fuzz._draw has it; every third such draw keeps W = 0
    e = (seed // 16) % 2
    if seg(d) and d.L > df.UNIT_SITES and d.W == 0 and rng.integers(3):
        u = int(rng.integers(1, (d.L - 1) // df.UNIT_SITES + 1))
        d.W = u * df.UNIT_SITES - e
        if d.lens is not None:
            d.lens = np.maximum(d.lens, d.W + 1 + rng.integers(0, d.L - d.W, size=d.N))
            if d.lens_mode == 2:
                d.lens[d.inds[0]] = d.W + 1
                if d.S > 1 and d.inds[1] != d.inds[0]:
                    d.lens[d.inds[1]] = d.L
    # a bin longer than two units: its owner walks down through two neighbours' blocks
    if seg(d) and d.L - d.W > 2 * df.UNIT_SITES and rng.integers(2):
        d.bin = int(rng.choice([1025, 1500, d.L - d.W]))
    d.form = FORMS[(seed + seed // 7) % len(FORMS)]  # stratified: every form within 7 seeds, against every K within 70
    d.v_rows = d.B > 1 and bool(rng.integers(4))
    rows = d.B if d.v_rows else 1
    v = _value_rows(rng, d.form, rows, d.K)
    assert np.abs(v).max(initial=0.0) <= 1.0
    d.raw = seed % 3 == 0
    d.map_a = d.map_c = None
    if not d.raw:  # arbitrary units: a + c v per row
        d.map_c = 10.0 ** rng.uniform(-3.0, 4.0, size=rows)
        d.map_a = rng.choice([-1.0, 1.0], size=rows) * d.map_c * 10.0 ** rng.uniform(-1.0, 0.7, size=rows)
        v = d.map_a[:, None] + d.map_c[:, None] * v
    d.vals = v if d.v_rows else v[0]
    # every other bin of one site becomes a few sites: there m2's cross terms are of the size of the sites' own variances
    if d.bin == 1 and seed % 2:
        d.bin = int(rng.choice([2, 7, 16]))
    return d


def vals_of(d, b):
    return d.vals[b] if d.v_rows else d.vals


def centre(d, b, pi_of=None):
    """-> (c_b, s_b, the row in [-1, 1] the kernel runs on) of particle b: ``PSMCKernel.bin_moments``' map in numpy float64, from
    the draw's own pi (the sum of the chunks' rows); a raw draw's row goes in as it is"""
    v = np.asarray(vals_of(d, b), float)
    if d.raw:
        return 0.0, 1.0, v
    pi = np.asarray(d.pp.pi[b if pi_of is None else pi_of], float).sum(0)
    lo = v.min()
    c = lo + ((v - lo) * pi).sum() / pi.sum()
    s = np.abs(v - c).max()
    row = np.clip((v - c) / s, -1.0, 1.0) if s > 0 else np.zeros_like(v)
    return float(c), float(s), row


def flat(d):
    """the kernel's row is all zeros: a zeros row, or through the API a row constant over the states"""
    return d.form == "zeros" or (not d.raw and d.form == "constant")


def describe(d):
    m = "" if d.raw else f" a={[float(f'{x:.3g}') for x in d.map_a]} c={[float(f'{x:.3g}') for x in d.map_c]}"
    return (f"seed={d.seed} K={d.K} {'f64' if d.dbl else 'f32'}{'(redrawn)' if d.redrawn else ''} B={d.B} S={d.S} N={d.N} "
            f"inds={d.inds.tolist()} L={d.L} W={d.W} het={d.het} miss={d.miss} runs={int(d.runs)} {'chunk' if d.per_chunk else 'bcast'} "
            f"nrm={d.nrm} ws={d.ws} slab={d.slab} {'raw' if d.raw else 'api'} plan={d.plan} bin={d.bin} "
            f"lens={None if d.lens is None else d.lens.tolist()} values={d.form}{'[B,K]' if d.v_rows else '[K]'}{m}")


@functools.lru_cache(maxsize=None)
def draw(seed):
    """Deterministic, CPU only.  A float32 draw on which the float32 emulation of the oracle itself keeps less than the redraw
    cap / 5 is redrawn as float64."""
    d = _draw(seed, False)
    if not d.dbl and oracle(d)["redraw"] > 1.0:
        d = _draw(seed, True)
        d.redrawn = True
    return d


def manual_draw(K, dbl, data, inds, pp, W, vals, bin, lens=None, plan=None, nrm=4, seed=-1, map_a=None, map_c=None):
    """a draw with given fields (the fixed-shape GPU tests): one block per particle, pp [B, 1, K], a value row per particle
    [B, K]; no slabs; through the API with ``map_a`` / ``map_c`` ([B] each), else raw"""
    data = np.asarray(data, np.int8)
    d = df.Draw(seed=seed, kind=KIND, redrawn=False, K=K, Kc=min(k for k in df.COMPILED_K if k >= K), dbl=dbl, L=data.shape[1],
                B=pp.pi.shape[0], S=len(inds), N=data.shape[0], inds=np.asarray(inds), W=W, het=float("nan"), miss=float("nan"),
                runs=False, data=data, per_chunk=False, pp=pp, nrm=nrm, ws="none", ws_limit=None, raw=map_c is None, plan=plan,
                bin=bin, lens=None if lens is None else np.asarray(lens), lens_mode=0, values=None, marginals=True, form="signed",
                v_rows=True, map_a=map_a, map_c=map_c)
    d.slab = (d.B, d.S)
    v = np.asarray(vals, float)
    d.vals = v if map_c is None else np.asarray(map_a)[:, None] + np.asarray(map_c)[:, None] * v
    return d


# ------------------------------------------------------------------------------------------------- oracle and emulation
def moments32(pp, data, v, W, bins, length):
    """``moment_oracle.dense`` with every array and operation in float32 (the dense model is built in float64 and rounded once)
    for one value row v [K] and a tuple of bin sizes -> ([m1 [nbin] float32 per size], [m2 ...])"""
    f = np.float32
    A, e, a0 = sf._model32(pp)
    codes = vo._codes(data)
    L, K = len(codes), A.shape[0]
    al = np.empty((L + 1, K), f)
    al[0] = a0
    for t in range(L):
        a = (al[t] @ A) * e[codes[t]]
        al[t + 1] = a / a.sum(dtype=f)
    v = np.asarray(v, float).astype(f)
    zero, two = np.zeros(K, f), f(2.0)
    o1 = [np.zeros((L - W + bn - 1) // bn, f) for bn in bins]
    o2 = [np.zeros((L - W + bn - 1) // bn, f) for bn in bins]
    last = [{en: k for k, s, en in mo._bins(L, W, bn)} for bn in bins]
    first = [{s: k for k, s, en in mo._bins(L, W, bn)} for bn in bins]
    b = np.ones(K, f)
    q1, q2 = np.zeros((len(bins), K), f), np.zeros((len(bins), K), f)
    for t in range(L - 1, W - 1, -1):
        for g in range(len(bins)):
            if t in last[g]:
                q1[g] = 0.0
                q2[g] = 0.0
        et = e[codes[t]]
        vt = v if t < length else zero
        w0, w1, w2 = et * b, et * q1, et * q2
        q1 = (w1 + vt * w0) @ A.T
        q2 = (w2 + two * vt * w1 + vt * vt * w0) @ A.T
        b = A @ w0
        z = b.sum(dtype=f)
        b, q1, q2 = b / z, q1 / z, q2 / z
        if t < length:
            for g in range(len(bins)):
                if t in first[g]:
                    den = b @ al[t]
                    o1[g][first[g][t]] = (q1[g] @ al[t]) / den
                    o2[g][first[g][t]] = (q2[g] @ al[t]) / den
    assert all(x.dtype == f for x in o1 + o2) and q1.dtype == f and b.dtype == f
    return o1, o2


def err(x, ref):
    """the project's metric, per bin: |x - ref| / max(1, |ref|)"""
    x, ref = np.asarray(x, float), np.asarray(ref, float)
    return np.abs(x - ref) / np.maximum(1.0, np.abs(ref))


def site_sums(x, bin, nbin):
    """x [n] per scored site -> [nbin]: sums over every bin's sites"""
    pad = np.zeros(nbin * bin)
    pad[: len(x)] = x
    return pad.reshape(nbin, bin).sum(1)


def sequence_oracle(pp, data, v, W, bin, length, dbl):
    """-> {"m1", "m2" [nbin], "m1_site", "m2_site" [L - W] (bin 1), "ll", "n_own", and "E1", "E2" [nbin] + "m1_32", "m2_32"
    (float32 draws) or "floor" (m1, m2) + "m1_s", "m2_s" (float64 draws)} of one sequence"""
    (m1, m1s), (m2, m2s), ll = mo.dense(pp, data, v, W, (bin, 1), length)
    o = {"m1": m1, "m2": m2, "m1_site": m1s, "m2_site": m2s, "ll": ll, "n_own": max(length - W, 0)}
    if dbl:
        s1, s2 = mo.structured(pp, data, v, W, bin, length)
        o.update(m1_s=s1, m2_s=s2, floor=(float(err(s1, m1).max(initial=0.0)), float(err(s2, m2).max(initial=0.0))))
    else:
        (a1, a1s), (a2, _) = moments32(pp, data, v, W, (bin, 1), length)
        a1, a2 = a1.astype(float), a2.astype(float)
        by_site = site_sums(np.abs(a1s.astype(float) - m1s), bin, len(m1)) / np.maximum(1.0, np.abs(m1))
        o.update(m1_32=a1, m2_32=a2, E1=np.maximum(err(a1, m1), by_site), E2=err(a2, m2))
    return o


def own_counts(d, n_own):
    return sf.own_counts(d, n_own)


def scale_of(d, n_own):
    """[nbin]: what a bar measured at bins of <= 100 sites is multiplied by"""
    return np.maximum(1.0, own_counts(d, n_own) / BIN_SITES)


def bin_bars(o, d):
    """-> (bar of m1 [nbin], bar of m2 [nbin]) of one sequence, on |x - ref| / max(1, |ref|)"""
    s = scale_of(d, o["n_own"])
    if d.dbl:
        return tuple(np.maximum(bars.F64_MOMENT_BAR * s, 5.0 * o["floor"][i]) for i in range(2))
    return tuple(np.maximum(F32_FLAT_BAR * s, 5.0 * o[name]) for name in ("E1", "E2"))


def oracle(d, shared=None):
    """-> {"ll": [B, S], "seq": [B][S] sequence_oracle dicts, "maps": [B] (c_b, s_b, row), "redraw": the largest 5 x E over its
    cap (float32 draws)}; computed once per (parameter block, data row, own length, value row) and kept on the draw.  ``shared``:
    a dict that keeps the sequences between draws which share blocks, rows and value rows (the caller's keys)."""
    if getattr(d, "_oracle", None) is not None:
        return d._oracle
    seqs, out = {} if shared is None else shared, []
    maps = [centre(d, b) for b in range(d.B)]
    LL = np.empty((d.B, d.S))
    redraw = 0.0
    for b in range(d.B):
        out.append([])
        for s in range(d.S):
            length = d.row_len(s)
            key = d.block_id(b, s) + (int(d.inds[s]), length, b if d.v_rows or not d.raw else 0)
            if key not in seqs:
                seqs[key] = sequence_oracle(d.block(b, s), d.data[d.inds[s]], maps[b][2], d.W, d.bin, length, d.dbl)
            o = seqs[key]
            out[b].append(o)
            LL[b, s] = o["ll"]
            if not d.dbl and d.nbin:
                cap = df.F32_REDRAW_BAR * scale_of(d, o["n_own"])
                redraw = max(redraw, float((5.0 * np.maximum(o["E1"], o["E2"]) / cap).max()))
    d._oracle = {"ll": LL, "seq": out, "maps": maps, "redraw": redraw}
    return d._oracle


# ------------------------------------------------------------------------------------------------- candidates (CPU tests)
def api_outputs(d, m1, m2, maps):
    """``PSMCKernel.bin_moments``' mean and var of m1, m2 [B, S, nbin] under ``maps`` [B] (c, s, ..)"""
    n = np.array([own_counts(d, d.row_len(s) - d.W) for s in range(d.S)], float).reshape(d.S, d.nbin)
    c = np.array([m[0] for m in maps])[:, None, None]
    s = np.array([m[1] for m in maps])[:, None, None]
    return s * m1 + c * n[None], s * s * np.maximum(m2 - m1 * m1, 0.0)


def finish(d, ll, m1, m2, maps):
    cand = {"ll": np.array(ll, float), "dtype": "float64", "m1": m1, "m2": m2}
    if not d.raw:
        cand["mean"], cand["var"] = api_outputs(d, m1, m2, maps)
    return cand


def oracle_candidate(d, tag=""):
    """the oracle's own output (``tag`` = "_32": the float32 emulation's, "_s": the structured statement's) in the form of a call's"""
    o = oracle(d)
    m1, m2 = (np.array([[o["seq"][b][s][n + tag] for s in range(d.S)] for b in range(d.B)]).reshape(d.B, d.S, d.nbin) for n in ("m1", "m2"))
    return finish(d, o["ll"], m1, m2, o["maps"])


def moments_candidate(d, row_len=None, W=None, shift=0, values=None, m2=None, maps=None):
    """What a call of draw ``d`` returns if the rows' own lengths are ``row_len(s)`` (default: the draw's), the warm-up is ``W``,
    the bins lie ``shift`` sites to the right, the kernel's row of particle b is ``values(b)`` and its second moment is
    ``m2(o, b, s)`` of the sequence's {"m1", "m2", "m1_site", "m2_site"}; the API's mean and var under ``maps`` [B] (c, s, ..);
    ll is the oracle's.  Recomputed here, for this draw only."""
    W0 = (d.W if W is None else W) + shift
    o = oracle(d)
    n = [d.row_len(s) if row_len is None else int(row_len(s)) for s in range(d.S)]
    M1, M2 = np.zeros((d.B, d.S, d.nbin)), np.zeros((d.B, d.S, d.nbin))
    cache = {}
    for b in range(d.B):
        v = o["maps"][b][2] if values is None else values(b)
        for s in range(d.S):
            key = d.block_id(b, s) + (int(d.inds[s]), n[s])
            if key not in cache:
                (a1, a1s), (a2, a2s), _ = mo.dense(d.block(b, s), d.data[d.inds[s]], v, W0, (d.bin, 1), n[s])
                cache[key] = {"m1": a1, "m2": a2, "m1_site": a1s, "m2_site": a2s}
            q = cache[key]
            k = min(len(q["m1"]), d.nbin)
            M1[b, s, :k] = q["m1"][:k]
            M2[b, s, :k] = (q["m2"] if m2 is None else m2(q, b, s))[:k]
    return finish(d, o["ll"], M1, M2, o["maps"] if maps is None else maps)


# ------------------------------------------------------------------------------------------------- the comparator
def compare(oracle, cand, d):
    """-> (worst error / bar over everything compared, message, {"m1", "m2": worst raw errors}).  A ratio above 1 -- inf for a wrong
    shape or type, a non-finite value, a non-zero moment in a bin without a site of the row's own or at W = L, a row of zeros
    with a non-zero output, a constant row whose mean is not c n to the bit -- fails the draw."""
    ll = np.asarray(cand["ll"], float)
    if ll.shape != (d.B, d.S):
        return FAIL, f"ll shape {ll.shape}", {}
    if cand.get("dtype") != "float64":
        return FAIL, f"moments are {cand.get('dtype')}: float64 for either handle type", {}
    names = ("m1", "m2") if d.raw else ("m1", "m2", "mean", "var")
    x = {}
    for name in names:
        x[name], msg = sf._array(cand, name, (d.B, d.S, d.nbin), d)
        if msg:
            return FAIL, msg, {}
    if not np.isfinite(ll).all():
        return FAIL, "ll not finite", {}
    if d.W == d.L and (ll.any() or any(a.any() for a in x.values())):
        return FAIL, "W = L: the outputs and ll are not all 0", {}
    cnt = np.array([own_counts(d, d.row_len(s) - d.W) for s in range(d.S)], float).reshape(d.S, d.nbin)
    for name in names:
        if x[name][:, cnt == 0].any():
            return FAIL, f"{name} of a bin without a site of the row's own is not 0", {}
    if flat(d):
        for name in ("m1", "m2") if d.raw else ("m1", "m2", "var"):
            if x[name].any():
                return FAIL, f"a row of zeros and a {name} that is not exactly 0", {}
        if not d.raw:
            for b in range(d.B):
                if not np.array_equal(x["mean"][b], float(vals_of(d, b)[0]) * cnt):
                    return FAIL, f"particle {b}: the mean of a constant row is not c n to the bit", {}
    if not d.raw and (x["var"] < 0).any():
        return FAIL, "var < 0", {}
    j = sf._Judge()
    sf._hold_ll(j, d, ll, oracle["ll"])
    raw = {"m1": 0.0, "m2": 0.0}
    if not d.nbin:
        return j.worst, j.msg, raw
    for b in range(d.B):
        c, sc, _ = oracle["maps"][b]
        for s in range(d.S):
            o, where, n = oracle["seq"][b][s], f"(particle {b}, chunk {s})", cnt[s]
            bar = bin_bars(o, d)
            for i, name in enumerate(("m1", "m2")):
                e = err(x[name][b, s], o[name])
                raw[name] = max(raw[name], float(e.max()))
                k = int((e / bar[i]).argmax())
                j.hold(float((e / bar[i]).max()), f"{name} of {where}, bin {k}: error {e[k]:.3e}, bar {bar[i][k]:.3e}")
            a1, a2 = x["m1"][b, s], x["m2"][b, s]
            j.hold(float((-a2 / bar[1]).max()), f"{where}: m2 < 0 by more than its bar")
            over = np.maximum(np.abs(a1) - n * (1.0 + bar[0]), a2 - n * n * (1.0 + bar[1]))
            j.hold(float(np.where(over > 0, np.inf, 0.0).max()), f"{where}: |m1| > n or m2 > n^2 by more than the bars")
            if not d.raw:
                r1, r2 = o["m1"], o["m2"]
                dd = bar[0] * np.maximum(1.0, np.abs(r1))
                t_mean = sc * dd + (d.K + 8) * EPS64 * (np.abs(sc * r1) + np.abs(vals_of(d, b)).max() * n)
                t_var = sc * sc * (bar[1] * np.maximum(1.0, r2) + 2.0 * np.abs(r1) * dd + dd * dd + 4.0 * EPS64 * (np.abs(r2) + r1 * r1))
                e_mean = np.abs(x["mean"][b, s] - (sc * r1 + c * n))
                e_var = np.abs(x["var"][b, s] - sc * sc * np.maximum(r2 - r1 * r1, 0.0))
                for name, e, t in (("mean", e_mean, t_mean), ("var", e_var, t_var)):
                    r = np.where(n > 0, e / np.where(t > 0, t, 1.0), 0.0)
                    r = np.where((t <= 0) & (e > 0), np.inf, r)
                    k = int(r.argmax())
                    j.hold(float(r.max()), f"{name} of {where}, bin {k}: error {e[k]:.3e}, allowed {t[k]:.3e}")
    return j.worst, j.msg, raw
