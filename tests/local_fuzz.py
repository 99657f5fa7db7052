"""Seeded random draws for the local likelihood-ratio scan (``phk_local_ratio``), a float32 emulation of its float64 dense
oracle, and the comparator that holds a candidate output against the oracle.  Test infrastructure only, CPU only; used by
tests/test_local_fuzz.py (the GPU tests and the CPU self-tests share the comparator).

A draw is the posterior draw of tests/decode_fuzz.py from a random stream of its own, the sweep draws' lens modes and long-bin
rule (tests/sweep_fuzz.py), and an alternative: its form (ALT_FORMS) and its layout (ALT_LAYOUTS: one block for everything,
one per particle, one per chunk position, one per sequence), both stratified by seed so that neither is tied to K
(seed % 10) or to the float type ((seed // 10) % 2).

Bars.  Nothing here is measured on the kernels.  The float64 reference is local_oracle.dense with the draw's own lens; the
metric is the project's, |x - ref| / max(1, |ref|) over the finite entries.
* float64, per sequence: max(local_bars.F64_LOCAL_BAR, 10 x S), S the error of local_oracle.structured (the kernel's form in
  float64 loops) on that sequence against the dense oracle, at the draw's bin and at bin 1: the project's "10 x the floor of
  the kernel's form", per sequence.  tests/test_local_fuzz.py checks S <= F64_LOCAL_BAR on every float64 default draw, so the bar
  is never more than 10 x the project's.
* float32, per sequence: max(local_bars.F32_LOCAL_BAR, 5 x E), E the error of ``local32`` (the dense oracle with every array
  and operation in float32; the log scale is accumulated in float64) on that sequence, at the draw's bin and at bin 1, whichever
  is larger (the argument of sweep_fuzz.tract32).  A float32 draw with 5 x E above decode_fuzz.F32_REDRAW_BAR is redrawn as
  float64.
* Exact properties, whatever the bars: shape and type; no NaN, no +inf; the set of -inf entries is the oracle's; a bin without
  a site of the row's own is exactly 0; an alternative that is the fitted block gives exactly 0 everywhere.
* ``ll``: as sweep_fuzz._hold_ll holds it.
"""

from __future__ import annotations

import functools

import numpy as np

import decode_fuzz as df
import local_bars
import local_oracle as lo
import sweep_fuzz as sf
import viterbi_oracle as vo
from oracle import psmc_numpy as pn

FAIL = df.FAIL
ALT_FORMS = ("same", "theta4", "theta_quarter", "rho_quarter", "ne2", "other", "blockout", "indicator", "tiny_het", "dead_het")
ALT_LAYOUTS = ("one", "particle", "chunk", "both")
SCALED = {"theta4": ("theta", 4.0), "theta_quarter": ("theta", 0.25), "rho_quarter": ("rho", 0.25), "ne2": ("ne", 2.0)}
F32_LINEAR = 88.8  # log of the largest float32: a log ratio beyond it is outside float32's linear range


# ------------------------------------------------------------------------------------------------- the draw
def _scaled_population(K, n, seed, what, s, fitted):
    """the population behind the fitted blocks (decode_fuzz._population) with theta, rho or the sizes scaled -> pn.PP [n, K];
    the unscaled population must give the fitted blocks bit for bit"""
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel, SizeHistory
    from phlash_amd.synth import particle_population

    tmpl, x = particle_population(K, n, seed=seed, sigma=0.25)
    dm = tmpl.from_flat(x).to_dm()
    base = PSMCParams.from_dm(dm)
    for a, ref in zip(base, fitted):
        assert np.array_equal(np.asarray(a.numpy(), float).reshape(ref.shape), ref), "the population behind the draw moved"
    if what == "theta":
        dm = DemographicModel(eta=dm.eta, theta=dm.theta * s, rho=dm.rho)
    elif what == "rho":
        dm = DemographicModel(eta=dm.eta, theta=dm.theta, rho=dm.rho * s)
    else:
        dm = DemographicModel(eta=SizeHistory(t=dm.eta.t, c=dm.eta.c / s), theta=dm.theta, rho=dm.rho)
    return pn.PP(*(np.asarray(a.numpy(), float) for a in PSMCParams.from_dm(dm)))


class Draw(df.Draw):
    def alt_id(self, b, s):
        Ba, Sa = self.alt.d.shape[:2]
        return (b if Ba > 1 else 0, s if Sa > 1 else 0)

    def alt_block(self, b, s):
        """the alternative block of (particle b, chunk position s) as a pn.PP of [K] arrays"""
        return pn.PP(*(a[self.alt_id(b, s)] for a in self.alt))

    def slab_origin(self, b, s):
        """(b0, s0) of the slab that holds sequence (b, s)"""
        nb, ns = self.slab
        return (b // nb * nb, s // ns * ns)


def _draw(seed, force_dbl):
    base, rng = df._draw(seed, "local", force_dbl, with_rng=True)
    d = Draw(**vars(base))
    d.values, d.marginals = None, True  # (not used)
    sf.lens_and_long_bin(d, rng)
    # form and layout: every form within ten seeds and in both float types within twenty, every layout within four; the
    # decade moves both, so that neither stays with a K or a float type
    d.alt_form = ALT_FORMS[(seed % 10 + 3 * (seed // 10)) % 10]
    d.alt_layout = ALT_LAYOUTS[(seed + seed // 10 + seed // 40) % 4]
    if d.alt_form == "dead_het" and d.L - d.W >= 2:
        # a het forbids the data: at least two bins, every row with a het at its first scored site and none in the last bin,
        # so that rows hold -inf and finite bins side by side
        d.bin = min(d.bin, (d.L - d.W + 1) // 2)
        d.data[:, d.W] = 1
        tail = d.data[:, d.W + (d.nbin - 1) * d.bin :]
        tail[tail == 1] = 0
    B, S, K = d.B, d.S, d.K
    Sp = S if d.per_chunk else 1
    if d.alt_form == "same":
        d.alt_layout = "both" if d.per_chunk else "particle"  # the fitted layout
        d.alt = pn.PP(*(a.copy() for a in d.pp))
        return d
    Ba = B if d.alt_layout in ("particle", "both") else 1
    Sa = S if d.alt_layout in ("chunk", "both") else 1
    if d.alt_form == "other":
        pop = df._population(K, Ba * Sa, seed=7000 + seed)  # independent models, all different
        d.alt = pn.PP(*(a.reshape(Ba, Sa, K) for a in pop))
        return d
    if d.alt_form in SCALED:
        what, s = SCALED[d.alt_form]
        full = _scaled_population(K, B * Sp, 100 + seed, what, s, [a.reshape(B * Sp, K) for a in d.pp])
        full = pn.PP(*(a.reshape(B, Sp, K) for a in full))
    else:
        full = d.pp
    # a derived form takes the fitted block at (b or 0, s or 0)
    bi = np.arange(Ba)[:, None]
    si = (np.arange(Sa) if d.per_chunk else np.zeros(Sa, int))[None, :]
    alt = pn.PP(*(np.array(a[bi, si]) for a in full))
    if d.alt_form == "blockout":
        alt = alt._replace(emis0=np.ones_like(alt.emis0), emis1=np.ones_like(alt.emis1))
    elif d.alt_form == "indicator":  # a prefix of 1 .. K states, one per alternative block
        c = rng.integers(1, K + 1, size=(Ba, Sa))
        m = (np.arange(K)[None, None, :] < c[..., None]).astype(float)
        alt = alt._replace(emis0=alt.emis0 * m, emis1=alt.emis1 * m)
    elif d.alt_form == "tiny_het":  # below RATIO_MIN_EMIS0: the alternative lane runs unfolded beside a folded fitted lane
        alt = alt._replace(emis1=alt.emis1 * 2.0 ** -70)
    elif d.alt_form == "dead_het":
        alt = alt._replace(emis1=np.zeros_like(alt.emis1))
    d.alt = alt
    return d


def describe(d):
    s = (f"seed={d.seed} K={d.K} {'f64' if d.dbl else 'f32'}{'(redrawn)' if d.redrawn else ''} B={d.B} S={d.S} N={d.N} "
         f"inds={d.inds.tolist()} L={d.L} W={d.W} het={d.het} miss={d.miss} runs={int(d.runs)} {'chunk' if d.per_chunk else 'bcast'} "
         f"nrm={d.nrm} ws={d.ws} {'raw' if d.raw else 'api'} plan={d.plan} bin={d.bin} lens={None if d.lens is None else d.lens.tolist()}")
    return s + f" alt={d.alt_form} [{'x'.join(map(str, d.alt.d.shape[:2]))}] ({d.alt_layout})"


@functools.lru_cache(maxsize=None)
def draw(seed):
    """Deterministic, CPU only.  A float32 draw on which the float32 emulation of the oracle itself keeps less than the redraw
    cap / 5 is redrawn as float64."""
    d = _draw(seed, False)
    if not d.dbl and oracle(d)["redraw"] > 1.0:
        d = _draw(seed, True)
        d.redrawn = True
    return d


# ------------------------------------------------------------------------------------------------- float32 emulation
def local32(pp, alt, data, W, bins, length):
    """``local_oracle.dense`` in float32 for one alternative and a tuple of bin sizes -> [logratio [nbin] float64 per size].
    The dense models are built in float64 and rounded once; q is normalised to its own float32 sum at every site and the log
    of what is taken out of it is accumulated in float64."""
    f = np.float32
    A, e, a0 = sf._model32(pp)
    Aa = pn.dense_from_pp(alt).astype(f)
    ea = [np.asarray(alt.emis0, float).astype(f), np.asarray(alt.emis1, float).astype(f), np.ones(A.shape[0], f)]
    codes = vo._codes(data)
    L, K = len(codes), A.shape[0]
    al = np.empty((L + 1, K), f)
    al[0] = a0
    for t in range(L):
        a = (al[t] @ A) * e[codes[t]]
        al[t + 1] = a / a.sum(dtype=f)
    G = len(bins)
    out = [np.zeros((L - W + bn - 1) // bn) for bn in bins]
    last = [{en: k for k, s, en in lo._bins(L, W, bn)} for bn in bins]
    first = [{s: k for k, s, en in lo._bins(L, W, bn)} for bn in bins]
    b = np.ones(K, f)
    q = np.zeros((G, K), f)
    lq = np.zeros(G)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(L - 1, W - 1, -1):
            for g in range(G):
                if t in last[g]:
                    q[g] = b
                    lq[g] = 0.0
            et = e[codes[t]]
            q = (ea[codes[t]] * q) @ Aa.T if t < length else (et * q) @ A.T
            b = A @ (et * b)
            z = b.sum(dtype=f)
            b = b / z
            zq = q.sum(-1, dtype=f)
            q = np.where(zq[:, None] > 0, q / np.where(zq > 0, zq, f(1))[:, None], f(0)).astype(f)
            lq = lq + np.log(zq.astype(float)) - np.log(float(z))
            if t < length:
                for g in range(G):
                    if t in first[g]:
                        out[g][first[g][t]] = lq[g] + np.log(float(q[g] @ al[t])) - np.log(float(b @ al[t]))
    return out


# ------------------------------------------------------------------------------------------------- oracle of a draw
def err_of(x, ref):
    """the project's metric over the finite entries of the reference (the -inf entries are held exactly)"""
    fin = np.isfinite(ref) & np.isfinite(x)
    return float((np.abs(x[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max(initial=0.0))


def oracle(d):
    """-> {"ll": [B, S], "seq": [B][S] dict of the sequence's reference (``ratio`` [nbin], ``cnt`` [nbin] own sites per bin,
    float32 draws: ``E``, float64 draws: ``S``), "redraw": the largest 5 x E over its cap (float32 draws)}; computed once per (fitted block,
    alternative block, data row, own length) and kept on the draw"""
    if getattr(d, "_oracle", None) is not None:
        return d._oracle
    seqs, out = {}, []
    LL = np.empty((d.B, d.S))
    redraw = 0.0
    for b in range(d.B):
        out.append([])
        for s in range(d.S):
            row, length = d.data[d.inds[s]], d.row_len(s)
            key = d.block_id(b, s) + d.alt_id(b, s) + (int(d.inds[s]), length)
            if key not in seqs:
                q, alt = d.block(b, s), d.alt_block(b, s)
                o = {"cnt": sf.own_counts(d, length - d.W)}
                if d.dbl:
                    (r, r1), o["ll"] = lo.dense(q, alt, row, d.W, (d.bin, 1), length)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        e, e1 = lo.structured(q, alt, row, d.W, (d.bin, 1), length)
                    same = np.array_equal(np.isneginf(e), np.isneginf(r)) and np.array_equal(np.isneginf(e1), np.isneginf(r1))
                    ok = same and not (np.isnan(e).any() or np.isnan(e1).any() or np.isposinf(e).any() or np.isposinf(e1).any())
                    o["ratio"] = r
                    o["S"] = max(err_of(e, r), err_of(e1, r1)) if ok else float("inf")  # (held by test_reference_alone_conditions)
                else:
                    (r, r1), o["ll"] = lo.dense(q, alt, row, d.W, (d.bin, 1), length)
                    e, e1 = local32(q, alt, row, d.W, (d.bin, 1), length)
                    same = np.array_equal(np.isneginf(e), np.isneginf(r)) and np.array_equal(np.isneginf(e1), np.isneginf(r1))
                    ok = same and not (np.isnan(e).any() or np.isnan(e1).any() or np.isposinf(e).any() or np.isposinf(e1).any())
                    o["ratio"], o["ratio32"] = r, e
                    o["E"] = max(err_of(e, r), err_of(e1, r1)) if ok else float("inf")  # (float32 loses a -inf: redrawn)
                    redraw = max(redraw, 5.0 * o["E"] / df.F32_REDRAW_BAR)
                if d.alt_form == "same":  # by definition; the dense statement steps q and beta through different products
                    assert np.abs(o["ratio"]).max(initial=0.0) < 1e-12
                    o["ratio"] = np.zeros_like(o["ratio"])
                seqs[key] = o
            out[b].append(seqs[key])
            LL[b, s] = seqs[key]["ll"]
    d._oracle = {"ll": LL, "seq": out, "redraw": redraw}
    return d._oracle


# ------------------------------------------------------------------------------------------------- candidates (CPU tests)
def _f(d):
    return "float64" if d.dbl else "float32"


def candidate(d, ll=None, row_len=None, alt_of=None, shift=0):
    """what a call of draw ``d`` returns if it computes the dense oracle with the rows' own lengths ``row_len(s)`` (default: the
    draw's), the alternative block ``alt_of(b, s)`` (default: the draw's) and the bins moved ``shift`` sites to the right"""
    R = np.zeros((d.B, d.S, d.nbin))
    cache = {}
    for b in range(d.B):
        for s in range(d.S):
            n = d.row_len(s) if row_len is None else int(row_len(s))
            ab = d.alt_id(b, s) if alt_of is None else alt_of(b, s)
            key = d.block_id(b, s) + tuple(ab) + (int(d.inds[s]), n)
            if key not in cache:
                alt = pn.PP(*(a[tuple(ab)] for a in d.alt))
                cache[key] = lo.dense(d.block(b, s), alt, d.data[d.inds[s]], d.W + shift, d.bin, n)[0]
            r = cache[key]
            R[b, s, : len(r)] = r[: d.nbin]
    return {"ll": np.array(oracle(d)["ll"] if ll is None else ll, float), "dtype": _f(d), "log_ratio": R}


def oracle_candidate(d):
    """the oracle's own output in the form of a call's"""
    o = oracle(d)
    R = np.array([[o["seq"][b][s]["ratio"] for s in range(d.S)] for b in range(d.B)]).reshape(d.B, d.S, d.nbin)
    return {"ll": o["ll"].copy(), "dtype": _f(d), "log_ratio": R}


# ------------------------------------------------------------------------------------------------- comparator
def compare(oracle, cand, d):
    """-> (worst error / bar over everything compared, message, {"ratio": worst raw error}).  A ratio above 1 -- inf for a wrong
    shape or type, a NaN, a +inf, a -inf where the oracle has none or none where it has one, a broken exact zero -- fails the
    draw."""
    ll = np.asarray(cand["ll"], float)
    if ll.shape != (d.B, d.S):
        return FAIL, f"ll shape {ll.shape}", {}
    if cand.get("dtype") != _f(d):
        return FAIL, f"outputs are {cand.get('dtype')}, the handle's type is {_f(d)}", {}
    x = np.asarray(cand["log_ratio"], float)
    if x.shape != (d.B, d.S, d.nbin):
        return FAIL, f"log_ratio shape {x.shape}, expected {(d.B, d.S, d.nbin)}", {}
    if np.isnan(x).any() or np.isposinf(x).any():
        return FAIL, "log_ratio has a NaN or a +inf", {}
    j = sf._Judge()
    sf._hold_ll(j, d, ll, oracle["ll"])
    raw = {"ratio": 0.0}
    if not d.nbin:
        return j.worst, j.msg, raw
    if d.alt_form == "same" and (x != 0).any():
        return FAIL, f"alternative = fitted and a log ratio that is not exactly 0 ({x[x != 0][0]!r})", raw
    for b in range(d.B):
        for s in range(d.S):
            o, where = oracle["seq"][b][s], f"(particle {b}, chunk {s})"
            ref = o["ratio"]
            if (x[b, s][o["cnt"] == 0] != 0).any():
                return FAIL, f"{where}: a bin without a site of the row's own is not exactly 0", raw
            if not np.array_equal(np.isneginf(x[b, s]), np.isneginf(ref)):
                k = int(np.flatnonzero(np.isneginf(x[b, s]) != np.isneginf(ref))[0])
                return FAIL, f"{where}, bin {k}: {x[b, s, k]!r} where the oracle has {ref[k]!r}", raw
            err = err_of(x[b, s], ref)
            raw["ratio"] = max(raw["ratio"], err)
            if d.dbl:
                bar = max(local_bars.F64_LOCAL_BAR, 10.0 * o["S"])
            else:
                bar = max(local_bars.F32_LOCAL_BAR, 5.0 * o["E"])
            j.hold(err / bar, f"log ratio of {where}: error {err:.3e}, bar {bar:.3e}")
    return j.worst, j.msg, raw
