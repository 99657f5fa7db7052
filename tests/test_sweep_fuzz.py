"""The transition, predictive and tract sweeps (phk_transitions / phk_predictive / phk_tracts) on seeded random draws
(tests/sweep_fuzz.py) against their float64 oracles.

CPU: what the bars need from the references alone (the float32 redraw share, every float32 emulation inside its own comparator),
the coverage of the default seeds, and the comparators against the oracle's own output with one fault injected.  GPU: one call
per draw through ``PSMCKernel`` or the raw ``HipEngine`` method, held to the comparators, to bitwise repeatability, to the
gradient call's bits and plan around it, and to ``phk_posterior``'s ll.
``pytest -s -m gpu tests/test_sweep_fuzz.py`` prints one ``fuzz`` line per draw and a summary (profiles/sweep_fuzz.txt).
"""

from __future__ import annotations

import os
import time
import warnings

import numpy as np
import pytest

import decode_fuzz as df
import sweep_fuzz as sf
import test_decode_fuzz as tdf

DEFAULT_SEEDS = 64  # the smallest count at which every kind draws the whole list of test_default_seeds_cover_the_list
# draws that found a bug, kept by name whatever the number of seeds run: name -> (kind, seed)
REGRESSIONS: dict = {}
N_SEEDS = int(os.environ.get("PHK_SWEEP_FUZZ_SEEDS", str(DEFAULT_SEEDS)))


def _defaults(kind):
    return [sf.draw(seed, kind) for seed in range(DEFAULT_SEEDS)]


# ------------------------------------------------------------------------------------------------- CPU
def _emulated(d):
    """the float32 emulation's output in the form of a call's"""
    o = sf.oracle(d)
    per = lambda f: [[f(d.block(b, s), d.data[d.inds[s]], b, s) for s in range(d.S)] for b in range(d.B)]  # noqa: E731
    if d.kind == "transitions":
        return sf.transitions_candidate(d, per(lambda q, row, b, s: sf.trans32(q, row, d.W).astype(float)), o["ll"])
    if d.kind == "predictive":
        ps = per(lambda q, row, b, s: sf.loo32(q, row, d.W))
        return sf.predictive_candidate(d, [[x[0].astype(float) for x in r] for r in ps], [[x[1].astype(float) for x in r] for r in ps], o["ll"])
    P = per(lambda q, row, b, s: sf.tract32(q, row, sf.weight_row(d, b), d.W, (d.bin,), d.row_len(s))[0].astype(float))
    return {"ll": o["ll"], "dtype": "float32", "prob": np.array(P).reshape(d.B, d.S, d.nbin)}


@pytest.mark.parametrize("kind", sf.KINDS)
def test_reference_alone_conditions(kind):
    """The bars are derived from the references: this is where they are checked against the references, without a kernel.
    Float32 draws that float32 itself cannot hold are redrawn as float64 -- at most 5 % of them; every float32 emulation sits
    inside its own bars (the oracle's ll beside it)."""
    draws = _defaults(kind)
    f32_default = [d for d in draws if not (d.seed // 10) % 2]
    redrawn = [d.seed for d in f32_default if d.redrawn]
    kept = [d for d in draws if not d.dbl]
    worst = max((sf.oracle(d)["redraw"] for d in kept), default=0.0)
    print(f"{kind}: {len(redrawn)} of {len(f32_default)} float32 draws redrawn as float64 (seeds {redrawn}); "
          f"largest 5 x E kept is {worst:.3f} of its cap")
    assert len(redrawn) <= 0.05 * len(f32_default), redrawn
    top = 0.0
    for d in kept:
        ratio, msg, _ = sf.compare(sf.oracle(d), _emulated(d), d)
        assert ratio <= 1.0, (sf.describe(d), msg)
        top = max(top, ratio)
    print(f"{kind}: the float32 emulation on {len(kept)} float32 draws: worst ratio to its bars {top:.3f}")


def _features(d):
    f = tdf._features(d)  # (the posterior draw's list)
    if d.plan is not None and d.plan[2] == 16 and d.dbl:
        f.add("T=16 f64")
    if d.lens is not None:
        own = [d.row_len(s) for s in range(d.S)]
        if len(set(own)) > 1 and d.W + 1 in own:
            f.add("ragged lens with a row at W+1")
        if any(d.lens[d.inds[s]] != d.lens[s] for s in range(d.S)):
            f.add("lens differ by row and by position")
    if d.kind == "transitions":
        if not d.arrivals:
            f.add("arrivals off")
        if not d.changes:
            f.add("changes off")
    if d.kind == "tracts":
        f.add(f"weights {d.wform}")
        if d.w_rows and any(not np.array_equal(d.weights[0], d.weights[b]) for b in range(1, d.B)):
            f.add("weights [B, K] that differ")
            if d.ws == "particles":
                f.add("weights [B, K] with slabs of particles")
    return f


def _wanted(kind):
    want = {f"K={K} {t}" for K in df.KS for t in ("f32", "f64")} | {f"L={L}" for L in df.LS}
    want |= {"nrm=1", "nrm=2", "nrm=4", "slab=particles", "slab=chunks", "inds permuted", "inds repeated", "inds subset",
             "per-chunk blocks differ", "W=L-1", "W=L", "het=0", "missing runs", "T=16 f64", "R_forward=16 at K=16 f32",
             "segmented, >= 3 units", "bin ends on a unit's first site", "bin ends on a unit's last site",
             "bin > 512 under a segmented plan", "bin > L-W", "ragged lens with a row at W+1", "lens differ by row and by position"}
    if kind == "transitions":
        want |= {"arrivals off", "changes off"}
    if kind == "tracts":
        want |= {f"weights {w}" for w in sf.WFORMS} | {"weights [B, K] that differ", "weights [B, K] with slabs of particles"}
    return want


@pytest.mark.parametrize("kind", sf.KINDS)
def test_default_seeds_cover_the_list(kind):
    seen = set()
    for d in _defaults(kind):
        seen |= _features(d)
    want = _wanted(kind)
    assert not want - seen, f"the default {kind} seeds never draw: {sorted(want - seen)}"


def _first(kind, pred):
    for d in _defaults(kind):
        if pred(d):
            return d
    raise AssertionError("no default draw fits: change the draw")


def _per(o, d, name):
    return [[o["seq"][b][s][name].copy() for s in range(d.S)] for b in range(d.B)]


def _shift(G):  # bin boundaries one site to the right
    return [[np.concatenate([g[1:], g[-1:]]) for g in row] for row in G]


def _block(G, d):  # one 8-site block's contribution taken from its neighbour
    G = [[g.copy() for g in row] for row in G]
    t = (d.row_len(d.S - 1) - d.W) // 2 // 8 * 8
    G[-1][-1][t : t + 8] = G[-1][-1][t + 8 : t + 16]
    return G


def _swap_chunks(cand, d):  # two chunks' outputs swapped
    s0 = [s for s in range(d.S) if d.inds[s] != d.inds[0]][0]
    out = dict(cand)
    for k, v in cand.items():
        if isinstance(v, np.ndarray):
            v = v.copy()
            v[:, [0, s0]] = v[:, [s0, 0]]
            out[k] = v
    return out


def _ragged(d):
    """a float32 draw with rows that differ, own lengths that differ by row and by position, and room for an 8-site block"""
    return (not d.dbl and d.S >= 2 and len(np.unique(d.inds)) >= 2 and d.L - d.W >= 60 and d.lens is not None
            and any(int(d.lens[s]) != d.row_len(s) for s in range(d.S)) and d.row_len(d.S - 1) - d.W >= 40)


def _fault_draw(kind, pred):
    """the first default draw that fits, with bins of 7 sites if its own are longer than 16 (a private copy then)"""
    d = _first(kind, lambda d: _ragged(d) and pred(d))
    if d.bin > 16:
        d = sf.draw.__wrapped__(d.seed, kind)
        d.bin, d._oracle = 7, None
    return d


def test_comparators_catch_seeded_faults():
    """The oracle's own output passes on every default draw's kind; with one fault injected it fails.  Float32 draws: the
    looser bars."""
    caught = []

    def check(kind, d, name, cand):
        ratio, msg, _ = sf.compare(sf.oracle(d), cand, d)
        print(f"{kind} fault '{name}' on seed {d.seed}: ratio {ratio:.3g} ({msg})")
        assert ratio > 1.0, (kind, name)
        caught.append((kind, name))

    by_position = lambda d: (lambda s: int(d.lens[s]))  # noqa: E731
    one_more = lambda d: (lambda s: min(d.row_len(s) + 1, d.L))  # noqa: E731

    # transitions
    d = _fault_draw("transitions", lambda d: d.arrivals and d.changes)
    o = sf.oracle(d)
    assert sf.compare(o, sf.oracle_candidate(d), d)[0] <= 1.0
    arr, ll = _per(o, d, "arr"), o["ll"]
    check("transitions", d, "bins shifted by one site", sf.transitions_candidate(d, _shift(arr), ll))
    check("transitions", d, "two chunks swapped", _swap_chunks(sf.oracle_candidate(d), d))
    check("transitions", d, "lens by position", sf.transitions_candidate(d, arr, ll, by_position(d)))
    check("transitions", d, "a site past a row's own length counted", sf.transitions_candidate(d, arr, ll, one_more(d)))
    check("transitions", d, "up and down swapped", sf.transitions_candidate(d, [[a[:, [0, 2, 1]] for a in row] for row in arr], ll))
    check("transitions", d, "an 8-site block from its neighbour", sf.transitions_candidate(d, _block(arr, d), ll))
    only_c = sf.draw.__wrapped__(d.seed, "transitions")  # ... and changes alone (a copy of the draw, arrivals off): up and down swapped
    only_c.arrivals, only_c.bin, only_c._oracle = False, d.bin, None
    check("transitions", only_c, "up and down swapped, changes alone",
          sf.transitions_candidate(only_c, [[a[:, [0, 2, 1]] for a in row] for row in arr], ll))
    bad = sf.oracle_candidate(d)
    bad["changes"] = None  # an output asked for is missing
    check("transitions", d, "changes missing", bad)

    # predictive (a draw with missing sites, so that the two het tracks differ)
    d = _fault_draw("predictive", lambda d: d.miss > 0)
    o = sf.oracle(d)
    good = sf.oracle_candidate(d)
    assert sf.compare(o, good, d)[0] <= 1.0
    ph, sc, ll = _per(o, d, "phet"), _per(o, d, "score"), o["ll"]
    check("predictive", d, "bins shifted by one site", sf.predictive_candidate(d, _shift(ph), _shift(sc), ll))
    check("predictive", d, "two chunks swapped", _swap_chunks(good, d))
    check("predictive", d, "lens by position", sf.predictive_candidate(d, ph, sc, ll, by_position(d)))
    check("predictive", d, "a site past a row's own length counted", sf.predictive_candidate(d, ph, sc, ll, one_more(d)))
    check("predictive", d, "het_observed and het_missing swapped", dict(good, het_observed=good["het_missing"], het_missing=good["het_observed"]))
    check("predictive", d, "an 8-site block from its neighbour", sf.predictive_candidate(d, _block(ph, d), _block(sc, d), ll))
    check("predictive", d, "float64 outputs from a float32 handle", dict(good, dtype="float64"))

    # tracts: a weight row per particle (no 8-site block here: a bin's value is no sum of per-site terms)
    d = _fault_draw("tracts", lambda d: d.w_rows and d.wform != "ones")
    o = sf.oracle(d)
    good = sf.oracle_candidate(d)
    assert sf.compare(o, good, d)[0] <= 1.0
    ll = o["ll"]
    check("tracts", d, "bins shifted by one site", sf.tracts_candidate(d, ll, shift=1))
    check("tracts", d, "two chunks swapped", _swap_chunks(good, d))
    check("tracts", d, "lens by position", sf.tracts_candidate(d, ll, row_len=by_position(d)))
    check("tracts", d, "a site past a row's own length counted", sf.tracts_candidate(d, ll, row_len=one_more(d)))
    check("tracts", d, "the weight row of particle 0 for every particle", sf.tracts_candidate(d, ll, weights=lambda b: d.weights[0]))
    d = _first("tracts", lambda d: d.wform == "ones" and d.nbin > 0)  # all ones: one ulp below 1 fails, whatever the bar
    good = sf.oracle_candidate(d)
    assert sf.compare(sf.oracle(d), good, d)[0] <= 1.0
    check("tracts", d, "all-ones weights, prob one ulp below 1", dict(good, prob=np.nextafter(good["prob"], 0.0)))
    assert len(caught) == 21

    # the oracle's own output passes on every default draw
    for kind in sf.KINDS:
        for d in _defaults(kind):
            ratio, msg, _ = sf.compare(sf.oracle(d), sf.oracle_candidate(d), d)
            assert ratio <= 1.0, (sf.describe(d), msg)


# ------------------------------------------------------------------------------------------------- GPU
STATS: dict = {}
RAW = {"transitions": ("arrivals", "changes"), "predictive": ("het", "score"), "tracts": ("prob",)}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if not STATS:
        return
    print("\nsweep fuzz summary (per kind and float type)")
    for (kind, ft), rows in sorted(STATS.items()):
        w = max(rows, key=lambda r: r["ratio"])
        line = f"  {kind} {ft}: {len(rows)} draws, worst error/bar {w['ratio']:.3f} (seed {w['seed']})"
        for name in RAW[kind]:
            line += f", worst {name} error {max(r.get(name, 0.0) for r in rows):.3e}"
        if ft == "f64":
            line += f", {sum(r['redrawn'] for r in rows)} of them float32 draws redrawn as float64"
        print(line)
    for kind in sf.KINDS:
        t = sum(r["time"] for (k, _), rows in STATS.items() if k == kind for r in rows)
        print(f"  wall time of test_{kind}_random_shapes: {t:.1f} s (oracles included)")


def _call(d, kern, eng, pp, P, inds):
    """-> (the call's device tensors as a tuple, ll first; the candidate the comparator reads)"""
    import torch

    lens_t = None if d.lens is None else torch.as_tensor(d.lens, dtype=torch.int64).cuda()
    host = lambda x: None if x is None else x.double().cpu().numpy()  # noqa: E731
    if d.kind == "transitions":
        if d.raw:
            ll, c, a = eng.transitions(P, inds, d.W, bin=d.bin, lens=lens_t, arrivals=d.arrivals, changes=d.changes)
        else:
            ll, c, a = kern.transitions(pp, d.inds, bin=d.bin, lens=d.lens, arrivals=d.arrivals)
        outs, cand = (ll, c, a), {"changes": host(c), "arrivals": host(a)}
    elif d.kind == "predictive":
        if d.raw:
            ll, track = eng.predictive(P, inds, d.W, bin=d.bin, lens=lens_t)
            ho, hm, sc = track[..., 0], track[..., 1], track[..., 2]
        else:
            ll, ho, hm, sc = kern.predictive(pp, d.inds, bin=d.bin, lens=d.lens)
        outs, cand = (ll, ho, hm, sc), {"het_observed": host(ho), "het_missing": host(hm), "score": host(sc)}
    else:
        if d.raw:
            ll, p = eng.tracts(P, inds, torch.as_tensor(d.weights, dtype=torch.float64).cuda(), d.W, bin=d.bin, lens=lens_t)
        else:
            ll, p = kern.tracts(pp, d.inds, weights=d.weights, bin=d.bin, lens=d.lens)
        outs, cand = (ll, p), {"prob": host(p)}
    assert ll.dtype == torch.float64
    types = {str(x.dtype).replace("torch.", "") for x in outs[1:] if x is not None}
    cand.update(ll=ll.cpu().numpy(), dtype=types.pop() if len(types) == 1 else str(sorted(types)))
    return outs, cand


def _sweep_draw(kind, seed, record=True):
    import torch

    t0 = time.perf_counter()
    d = sf.draw(seed, kind)
    o = sf.oracle(d)
    kern, eng, pp, P, inds = tdf._setup(d)
    forced = d.plan is not None
    if forced:
        eng.set_plan(1 if d.plan[0] == "segmented" else 0, *d.plan[1:])
        ll0, g0 = eng.run(P, inds, d.W, grad=True)  # a gradient call before the sweep ...
        plan0 = eng.get_plan()
        if d.ws_limit is not None:
            assert eng.get_slab() == d.slab, (eng.get_slab(), d.slab)

    def call():
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out = _call(d, kern, eng, pp, P, inds)
            risk = eng.underflow_risk()
        assert not risk, "underflow flag raised on ordinary parameters"
        return out

    a, cand = call()
    ratio, msg, info = sf.compare(o, cand, d)
    print(f"fuzz {kind} {sf.describe(d)}: nbin={d.nbin} " + " ".join(f"{k} {v:.3e}" for k, v in info.items()) + f" worst error/bar {ratio:.3f}")
    assert ratio <= 1.0, msg
    b, _ = call()  # a repeat call: the same bits
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)
    if forced:
        ll1, g1 = eng.run(P, inds, d.W, grad=True)  # ... and after it: the same bits, the plan untouched
        assert torch.equal(ll0, ll1) and torch.equal(g0, g1)
        assert eng.get_plan() == plan0
    ll_post = eng.posterior(P, inds, d.W, bin=d.bin)[0]  # the same legs at the same plan, bin and W: ll to the bit
    assert torch.equal(a[0], ll_post), (a[0], ll_post)
    assert not eng.underflow_risk()
    if record:
        STATS.setdefault((kind, "f64" if d.dbl else "f32"), []).append(
            dict(info, seed=d.seed, ratio=ratio, redrawn=d.redrawn, time=time.perf_counter() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_transitions_random_shapes(seed):
    _sweep_draw("transitions", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_predictive_random_shapes(seed):
    _sweep_draw("predictive", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_tracts_random_shapes(seed):
    _sweep_draw("tracts", seed)


@pytest.mark.gpu
def test_regression_draws():
    """every pinned draw, whatever the number of seeds run (a loop: the table may be empty, and an empty parameter list skips)"""
    for name in sorted(REGRESSIONS):
        kind, seed = REGRESSIONS[name]
        _sweep_draw(kind, seed, record=False)
