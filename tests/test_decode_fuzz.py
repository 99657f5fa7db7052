"""Posterior and Viterbi decoding on seeded random draws (tests/decode_fuzz.py) against their float64 oracles.

CPU: what the bars need from the references alone (the float32 redraw cap, the float64 margin cap, the float32 emulation of the
structured max-product step inside the deficit bound), the coverage of the default seeds, and the comparators against the
oracle's own output with one fault injected.  GPU: one call per draw through ``PSMCKernel`` or the raw ``HipEngine`` method,
held to the comparators, to the identities that tie decoding to the shipped calls, and to bitwise repeatability.
``pytest -s -m gpu tests/test_decode_fuzz.py`` prints one ``fuzz`` line per draw and a summary (profiles/decode_fuzz.txt).
"""

from __future__ import annotations

import os
import time
import warnings

import numpy as np
import pytest

import decode_fuzz as df
import viterbi_oracle as vo

DEFAULT_SEEDS = 80
# draws that found a bug, kept by name whatever the number of seeds run: name -> (kind, seed)
REGRESSIONS = {
    # W = L (no scored site, nbin = 0): the empty outputs are null device pointers, and phk_posterior refused the call with
    # "mean and marginals are both NULL" instead of returning ll = 0 and the empty tensors
    "posterior_W_equals_L_api": ("posterior", 2),
    "posterior_W_equals_L_raw": ("posterior", 78),
}
N_SEEDS = int(os.environ.get("PHK_DECODE_FUZZ_SEEDS", str(DEFAULT_SEEDS)))


def _defaults(kind):
    return [df.draw(seed, kind) for seed in range(DEFAULT_SEEDS)]


# ------------------------------------------------------------------------------------------------- CPU
def test_reference_alone_conditions():
    """The bars are derived from the references: this is where they are checked against the references, without a kernel."""
    # posterior: float32 draws that float32 itself cannot hold are redrawn as float64 -- few; fb32 sits inside its own bar
    post = _defaults("posterior")
    f32_default = [d for d in post if not (d.seed // 10) % 2]
    redrawn = [d.seed for d in f32_default if d.redrawn]
    worst_E = max((float(df.oracle_posterior(d)["E"].max(initial=0.0)) for d in post if not d.dbl), default=0.0)
    print(f"posterior: {len(redrawn)} of {len(f32_default)} float32 draws redrawn as float64 (seeds {redrawn}); "
          f"largest fb32 error kept {worst_E:.3e}")
    assert len(redrawn) <= 0.05 * len(f32_default), redrawn
    for d in post:
        if d.dbl:
            continue
        o = df.oracle_posterior(d)
        g32 = [[df.fb32(d.block(b, s), d.data[d.inds[s]], d.W)[0].astype(float) for s in range(d.S)] for b in range(d.B)]
        ratio, msg, _ = df.compare_posterior(o, df.posterior_candidate(d, g32, o["ll"]), d)  # (fb32's gamma, the oracle's ll)
        assert ratio <= 1.0, (d.describe(), msg)
    # Viterbi, float64: sequences nearer to a tie than MIN_MARGIN are judged by the deficit rule only -- few
    vit = _defaults("viterbi")
    n64 = sum(d.B * d.S for d in vit if d.dbl)
    near = sum(int((df.oracle_viterbi(d)["margin"] < df.MIN_MARGIN).sum()) for d in vit if d.dbl)
    print(f"viterbi: {near} of {n64} float64 sequences have a margin below {df.MIN_MARGIN:g}")
    assert near <= 0.10 * n64
    # Viterbi, float32: the float32 emulation of the structured step stays inside the deficit bound on every draw (with the
    # unreported prefix counted as W steps: the prior state z_0 is maximised inside the first step and adds none)
    worst, nseq, ndiff = 0.0, 0, 0
    for d in vit:
        if d.dbl:
            continue
        o = df.oracle_viterbi(d)
        paths = [[None] * d.S for _ in range(d.B)]
        logp = np.empty((d.B, d.S))
        for b in range(d.B):
            for s in range(d.S):
                p, logp[b, s] = df.sv32(d.block(b, s), d.data[d.inds[s], : d.row_len(s)])
                paths[b][s] = p[d.W :]
        ratio, msg, info = df.compare_viterbi(o, df.viterbi_candidate(d, paths, logp), d)
        assert ratio <= 1.0, (d.describe(), msg)
        worst, nseq, ndiff = max(worst, ratio), nseq + info["n_seq"], ndiff + info["n_diff"]
    print(f"viterbi: sv32 on {nseq} float32 sequences: {ndiff} sites differ from the oracle's path, worst ratio to its bars {worst:.3f}")


def _mr_share(d):
    """share of the handle's sites in 8-site halves that are missing throughout (above 0.5 %: the *_mr kernels)"""
    n8 = (d.L // 8) * 8
    if n8 == 0:
        return 0.0
    return 8.0 * int((d.data[:, :n8].reshape(d.N, n8 // 8, 8) == -1).all(-1).sum()) / d.data.size


def _features(d):
    f = {f"K={d.K} {'f64' if d.dbl else 'f32'}", f"L={d.L}", f"nrm={d.nrm}", f"slab={d.ws}"}
    if (np.diff(d.inds) < 0).any():
        f.add("inds permuted")
    if len(np.unique(d.inds)) < d.S:
        f.add("inds repeated")
    if len(np.unique(d.inds)) < d.N:
        f.add("inds subset")
    if d.per_chunk and all(not np.array_equal(d.pp.d[b, 0], d.pp.d[b, 1]) for b in range(d.B)):
        f.add("per-chunk blocks differ")
    if d.W == d.L - 1 and d.L > 1:
        f.add("W=L-1")
    if d.W == d.L:
        f.add("W=L")
    if d.het == 0.0:
        f.add("het=0")
    if d.het >= 0.1:
        f.add("het>=0.1")
    if d.runs and _mr_share(d) > 0.005:
        f.add("missing runs")
    if d.kind == "viterbi":
        if d.lens is not None and len(set(d.row_len(s) for s in range(d.S))) > 1 and any(d.row_len(s) == d.W + 1 for s in range(d.S)):
            f.add("ragged lens with a row at W+1")
        return f
    n = d.L - d.W
    seg = d.plan is not None and d.plan[0] == "segmented"
    if seg and d.n_units >= 3:
        f.add("segmented, >= 3 units")
    if d.plan is not None and d.plan[2] == 16:
        f.add("T=16")
    if d.plan is not None and d.plan[3] == 16 and d.K == 16 and not d.dbl:
        f.add("R_forward=16 at K=16 f32")
    if seg and d.bin > df.UNIT_SITES and n > df.UNIT_SITES and d.n_units >= 2:
        f.add("bin > 512 under a segmented plan")
    if d.bin > n:
        f.add("bin > L-W")
    if seg and d.bin > 1 and d.n_units >= 2:
        ends = d.bin_ends()
        if ((ends % df.UNIT_SITES == 0) & (ends > 0)).any():
            f.add("bin ends on a unit's first site")
        if ((ends % df.UNIT_SITES == df.UNIT_SITES - 1) & (ends < d.L - 1)).any():
            f.add("bin ends on a unit's last site")
    if not d.marginals:
        f.add("mean only")
    if d.values is not None and d.values.ndim == 2 and d.B > 1:
        f.add("values [B, K]")
    return f


@pytest.mark.parametrize("kind", ["posterior", "viterbi"])
def test_default_seeds_cover_the_list(kind):
    want = {f"K={K} {t}" for K in df.KS for t in ("f32", "f64")} | {f"L={L}" for L in df.LS}
    want |= {"inds permuted", "inds repeated", "inds subset", "per-chunk blocks differ", "W=L-1", "het=0", "het>=0.1", "missing runs",
             "nrm=1", "nrm=2", "nrm=4", "slab=particles", "slab=chunks"}
    if kind == "posterior":
        want |= {"W=L", "segmented, >= 3 units", "T=16", "R_forward=16 at K=16 f32", "bin > 512 under a segmented plan", "bin > L-W",
                 "bin ends on a unit's first site", "bin ends on a unit's last site", "mean only", "values [B, K]"}
    else:
        want |= {"ragged lens with a row at W+1"}
    seen = set()
    for d in _defaults(kind):
        seen |= _features(d)
    assert not want - seen, f"the default {kind} seeds never draw: {sorted(want - seen)}"


def _first(kind, pred):
    for d in _defaults(kind):
        if pred(d):
            return d
    raise AssertionError("no default draw fits: change the draw")


def test_comparators_catch_seeded_faults():
    """The oracle's own output passes; with one fault injected it fails.  Float32 draws: the looser bars."""
    # posterior: a float32 draw with rows that differ, hets, a few hundred scored sites, small bins
    d = _first("posterior", lambda d: not d.dbl and d.marginals and d.S >= 2 and len(np.unique(d.inds)) >= 2 and d.L - d.W >= 200
               and 0.0 < d.het < 0.5 and d.bin <= 16)
    o = df.oracle_posterior(d)
    good = df.posterior_candidate(d, o["gamma"], o["ll"])
    assert df.compare_posterior(o, good, d)[0] <= 1.0

    def faulty(edit):
        G = [[g.copy() for g in row] for row in o["gamma"]]
        edit(G)
        return df.compare_posterior(o, df.posterior_candidate(d, G, o["ll"]), d)

    def shift(G):  # bin boundaries one site to the right
        for row in G:
            for i, g in enumerate(row):
                row[i] = np.concatenate([g[1:], g[-1:]])

    def swap(G):  # two chunks' outputs swapped
        s0, s1 = [s for s in range(d.S) if d.inds[s] != d.inds[0]][0], 0
        for row in G:
            row[s0], row[s1] = row[s1], row[s0]

    def block(G):  # gamma of one 8-site block taken from its neighbour
        t = (d.L - d.W) // 2 // 8 * 8
        G[-1][-1][t : t + 8] = G[-1][-1][t + 8 : t + 16]

    for name, edit in (("bins shifted by one site", shift), ("two chunks swapped", swap), ("an 8-site block from its neighbour", block)):
        ratio, msg, _ = faulty(edit)
        print(f"posterior fault '{name}' on seed {d.seed}: ratio {ratio:.3g} ({msg})")
        assert ratio > 1.0, name
    bad = dict(good, ll=good["ll"][:, ::-1].copy())  # ... and ll swapped between chunks
    assert df.compare_posterior(o, bad, d)[0] > 1.0

    # Viterbi: a float32 draw with rows of their own, different lengths
    d = _first("viterbi", lambda d: not d.dbl and d.lens is not None and d.L - d.W >= 30
               and any(d.lens[s] != d.row_len(s) for s in range(d.S)))
    o = df.oracle_viterbi(d)
    good = df.viterbi_candidate(d, o["path"], o["logp"])
    assert df.compare_viterbi(o, good, d)[0] <= 1.0
    # lens applied by position in inds instead of by data row
    paths = [[vo.viterbi(d.block(b, s), d.data[d.inds[s], : int(d.lens[s])], d.W, want_margin=False)[0] for s in range(d.S)]
             for b in range(d.B)]
    ratio, msg, _ = df.compare_viterbi(o, df.viterbi_candidate(d, paths, o["logp"]), d)
    print(f"viterbi fault 'lens by position' on seed {d.seed}: ratio {ratio:.3g} ({msg})")
    assert ratio > 1.0
    # a path tail that is not 255
    s = [s for s in range(d.S) if d.row_len(s) < d.L][0]
    bad = dict(good, path=good["path"].copy())
    bad["path"][0, s, -1] = 0
    assert df.compare_viterbi(o, bad, d)[0] > 1.0
    # two chunks swapped
    if d.S >= 2 and d.inds[0] != d.inds[-1]:
        bad = dict(good, path=good["path"][:, ::-1].copy(), logp=good["logp"][:, ::-1].copy())
        assert df.compare_viterbi(o, bad, d)[0] > 1.0
    # one backpointer flipped to the second-best predecessor, in float32 (the wider bound) and in float64
    for dbl in (False, True):
        d = _first("viterbi", lambda d: d.dbl == dbl and d.L - d.W >= 100 and 0.0 < d.het < 0.5)
        o = df.oracle_viterbi(d)
        paths = [list(row) for row in o["path"]]
        n = d.row_len(0)
        paths[0][0] = df.viterbi_with_flipped_pointer(d.block(0, 0), d.data[d.inds[0], :n], d.W, d.W + (n - d.W) // 2)
        assert not np.array_equal(paths[0][0], o["path"][0][0])
        ratio, msg, _ = df.compare_viterbi(o, df.viterbi_candidate(d, paths, o["logp"]), d)
        print(f"viterbi fault 'flipped backpointer' on seed {d.seed} ({'f64' if dbl else 'f32'}): ratio {ratio:.3g} ({msg})")
        assert ratio > 1.0


# ------------------------------------------------------------------------------------------------- GPU
STATS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if not STATS:
        return
    print("\ndecode fuzz summary (per kind and float type)")
    for (kind, ft), rows in sorted(STATS.items()):
        w = max(rows, key=lambda r: r["ratio"])
        line = f"  {kind} {ft}: {len(rows)} draws, worst error/bar {w['ratio']:.3f} (seed {w['seed']})"
        if kind == "posterior":
            line += f", worst |gamma - oracle| {max(r['gamma'] for r in rows):.3e}"
            if ft == "f64":
                line += f", {sum(r['redrawn'] for r in rows)} of them float32 draws redrawn as float64"
        else:
            nseq = sum(r["n_seq"] for r in rows)
            line += (f", worst deficit {max(r['deficit'] for r in rows):.3e}, {sum(r['n_diff'] for r in rows)} sites differ from the "
                     f"oracle's path, {sum(r['n_deficit_only'] for r in rows)} of {nseq} sequences judged by the deficit rule only")
        print(line)
    for kind in ("posterior", "viterbi"):
        t = sum(r["time"] for (k, _), rows in STATS.items() if k == kind for r in rows)
        print(f"  wall time of test_{kind}_random_shapes: {t:.1f} s (oracles included)")


def _setup(d):
    """-> (kernel object, engine, PSMCParams [B, S|1, K] on the host, P [B, S|1, 7, K] and inds on the device)"""
    import torch

    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # ("Performance is optimized when M=16")
        kern = get_kernel(d.K, d.data, double_precision=d.dbl, overlap=d.W)
    eng = kern._eng
    eng.set_rescale_interval(d.nrm)
    if d.ws_limit is not None:
        eng.set_workspace_limit(d.ws_limit)
    pp = PSMCParams(*(torch.as_tensor(a) for a in d.pp))
    P = torch.stack(list(pp), -2).cuda()
    inds = torch.as_tensor(d.inds, dtype=torch.int64).cuda()
    return kern, eng, pp, P, inds


def _record(d, t0, ratio, info, record=True):
    if record:
        STATS.setdefault((d.kind, "f64" if d.dbl else "f32"), []).append(
            dict(info, seed=d.seed, ratio=ratio, redrawn=d.redrawn, time=time.perf_counter() - t0))


def _posterior_draw(seed, record=True):
    import torch

    t0 = time.perf_counter()
    d = df.draw(seed, "posterior")
    o = df.oracle_posterior(d)
    kern, eng, pp, P, inds = _setup(d)
    forced = d.plan is not None
    if forced:
        eng.set_plan(1 if d.plan[0] == "segmented" else 0, *d.plan[1:])
        ll0, g0 = eng.run(P, inds, d.W, grad=True)  # a gradient call before the decode ...
        plan0 = eng.get_plan()
        if d.ws_limit is not None:
            assert eng.get_slab() == d.slab, (eng.get_slab(), d.slab)
    vals = None if d.values is None else torch.as_tensor(d.values, dtype=torch.float64).cuda()

    def call():
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            if d.raw:
                ll, mean, marg = eng.posterior(P, inds, d.W, values=vals, bin=d.bin, marginals=d.marginals, mean=vals is not None)
                risk = eng.underflow_risk()
            else:
                ll, mean, marg = kern.posterior(pp, d.inds, values=d.values, bin=d.bin, marginals=d.marginals)
                risk = eng.underflow_risk()
        assert not risk, "underflow flag raised on ordinary parameters"
        return ll, mean, marg

    a = call()
    cand = {"ll": a[0].cpu().numpy(), "mean": None if a[1] is None else a[1].double().cpu().numpy(),
            "marginals": None if a[2] is None else a[2].double().cpu().numpy()}
    ratio, msg, info = df.compare_posterior(o, cand, d)
    print(f"fuzz posterior {d.describe()}: nbin={d.nbin} max |gamma - oracle| {info.get('gamma', float('nan')):.3e} "
          f"worst error/bar {ratio:.3f}")
    assert ratio <= 1.0, msg
    b = call()  # a repeat call: the same bits
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)
    if forced:
        ll1, g1 = eng.run(P, inds, d.W, grad=True)  # ... and after it: the same bits, the plan untouched
        assert torch.equal(ll0, ll1) and torch.equal(g0, g1)
        assert eng.get_plan() == plan0
        ll_ng = eng.run(P, inds, d.W, grad=False)  # the forward leg's by-product is the no-gradient call's ll
        assert bool(((a[0] - ll_ng).abs() <= 1e-12 * ll_ng.abs()).all()), (a[0], ll_ng)
    assert not eng.underflow_risk()
    _record(d, t0, ratio, info, record)


def _viterbi_draw(seed, record=True):
    import torch

    t0 = time.perf_counter()
    d = df.draw(seed, "viterbi")
    o = df.oracle_viterbi(d)
    kern, eng, pp, P, inds = _setup(d)
    lens_t = None if d.lens is None else torch.as_tensor(d.lens, dtype=torch.int64).cuda()

    def call():
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            if d.raw:
                logp, path = eng.viterbi(P, inds, d.W, lens=lens_t)
            else:
                logp, path = kern.viterbi(pp, d.inds, lens=d.lens)
            risk = eng.underflow_risk()
        assert not risk, "underflow flag raised on ordinary parameters"
        return logp, path

    a = call()
    ratio, msg, info = df.compare_viterbi(o, {"logp": a[0].cpu().numpy(), "path": a[1].cpu().numpy()}, d)
    print(f"fuzz viterbi {d.describe()}: {info.get('n_diff', -1)} sites differ, deficit {info.get('deficit', float('nan')):.3e}, "
          f"worst error/bar {ratio:.3f}")
    assert ratio <= 1.0, msg
    b = call()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _record(d, t0, ratio, info, record)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_posterior_random_shapes(seed):
    _posterior_draw(seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_viterbi_random_shapes(seed):
    _viterbi_draw(seed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REGRESSIONS))
def test_regression_draws(name):
    kind, seed = REGRESSIONS[name]
    d = df.draw(seed, kind)
    if name.startswith("posterior_W_equals_L"):
        assert d.W == d.L and d.nbin == 0, "the draw changed: pin another seed with W = L"
    (_posterior_draw if kind == "posterior" else _viterbi_draw)(seed, record=False)
