"""Pair counts (phk_pair_counts) on seeded random draws (tests/pair_fuzz.py) against their float64 oracle.

CPU: what the bars need from the references alone (the float32 redraw share, the float32 emulation and the loop form inside
their own bars), the coverage of the default seeds, and the comparator against the oracle's own output with one fault injected.
GPU: one call per draw through ``PSMCKernel.pair_counts`` or the raw ``HipEngine`` method, held to the comparator, to bitwise
repeatability, to the gradient call's bits, plan and slab around it, to ``phk_posterior``'s ll and to the same bits with the
workspace limit lifted; more sequences than a wave and a workgroup hold; ``transition_counts`` over ragged contigs.
``pytest -s -m gpu tests/test_pair_fuzz.py`` prints one ``fuzz`` line per draw and a summary (profiles/pair_fuzz.txt).
"""

from __future__ import annotations

import os
import time
import warnings

import numpy as np
import pytest

import decode_fuzz as df
import pair_count_bars as bars
import pair_fuzz as pf
import test_decode_fuzz as tdf
from oracle import psmc_numpy as pn

DEFAULT_SEEDS = 64  # every item of test_default_seeds_cover_the_list is drawn within them
# draws that found a bug, kept by name whatever the number of seeds run: name -> seed
REGRESSIONS: dict = {}
N_SEEDS = int(os.environ.get("PHK_PAIR_FUZZ_SEEDS", str(DEFAULT_SEEDS)))


def _defaults():
    return [pf.draw(seed) for seed in range(DEFAULT_SEEDS)]


# ------------------------------------------------------------------------------------------------- CPU
def test_reference_alone_conditions():
    """The bars are derived from the references: this is where they are checked against the references, without a kernel.
    Float32 draws that float32 itself cannot hold are redrawn as float64 -- at most 5 % of them; the float32 emulation's summed
    matrix sits inside the float32 bars on every kept float32 draw, the loop form inside the float64 bars on every float64 draw
    (by construction of the bars' second terms: what is held here is that the bars are computed on the sequences compared)."""
    draws = _defaults()
    f32_default = [d for d in draws if not (d.seed // 10) % 2]
    redrawn = [d.seed for d in f32_default if d.redrawn]
    kept = [d for d in draws if not d.dbl]
    worst = max((pf.oracle(d)["redraw"] for d in kept), default=0.0)
    print(f"pairs: {len(redrawn)} of {len(f32_default)} float32 draws redrawn as float64 (seeds {redrawn}); "
          f"largest 5 x E / max(1, C) kept is {worst:.3f} of its cap")
    assert len(redrawn) <= 0.05 * len(f32_default), redrawn
    top, raw, flat = 0.0, (0.0, None), (0.0, None)
    for d in kept:
        o = pf.oracle(d)
        ratio, msg, info = pf.compare(o, pf.oracle_candidate(d, "C32"), d)
        assert ratio <= 1.0, (pf.describe(d), msg)
        top, raw = max(top, ratio), max(raw, (info["counts"], d.seed))
        for row in o["seq"]:
            for q in row:
                e = float((np.abs(q["C32"] - q["C"]) / np.maximum(1.0, q["C"])).max())
                flat = max(flat, (e / (bars.F32_COUNTS_BAR * pf.scale_of(q["n_own"])), d.seed))
    print(f"pairs: the float32 emulation on {len(kept)} float32 draws: worst ratio to its bars {top:.3f}; its summed matrix is at "
          f"most {raw[0]:.3e} off (seed {raw[1]}), {flat[0]:.2f} of the flat bar at most (seed {flat[1]})")
    top = (0.0, None)
    for d in draws:
        if not d.dbl:
            continue
        for row in pf.oracle(d)["seq"]:
            for q in row:
                assert q["floor"] <= pf.entry_bars(q, True), (pf.describe(d), q["floor"])
                top = max(top, (q["floor"] / (bars.F64_COUNTS_BAR * pf.scale_of(q["n_own"])), d.seed))
    print(f"pairs: the loop form on the float64 draws: at most {top[0]:.2f} of F64_COUNTS_BAR x scale (seed {top[1]})")


def _features(d):
    f = tdf._features(d)  # (the posterior draw's list; its bin and values items never come up at bin 1 without values)
    if d.het == 0.5:
        f.add("het=0.5")
    if d.miss == 0.3:
        f.add("miss=0.3")
    if d.raw:
        f.add("raw method")
    if d.plan is not None and d.plan[2] == 16 and d.dbl:
        f.add("T=16 f64")
    if d.lens is not None:
        own = [d.row_len(s) for s in range(d.S)]
        if len(set(own)) > 1 and d.W + 1 in own:
            f.add("ragged lens with a row at W+1")
        if any(d.lens[d.inds[s]] != d.lens[s] for s in range(d.S)):
            f.add("lens differ by row and by position")
    if pf.row_tiles(d) > 1 and d.ws != "none":
        f.add(f"row tiles under slab={d.ws}")
    if pf.row_tiles(d) > 1 and d.W < d.L:
        f.add(f"row tiles at nrm={d.nrm}")
        if d.dbl and d.plan is not None and d.plan[2] == 16:
            f.add("row tiles at T=16 f64")
    seg = pf.seg(d)
    if pf.matrix_path(d) and d.W < d.L:
        m = "matrix path: "
        if d.plan is not None:
            f.add(m + ("segmented, >= 3 units" if seg and d.n_units >= 3 else d.plan[0]))
            f.add(m + f"T={d.plan[2]}")
        f.add(m + f"nrm={d.nrm}")
        if "per-chunk blocks differ" in f:
            f.add(m + "per-chunk blocks")
        if d.ws != "none":
            f.add(m + f"slab={d.ws}")
    if not d.dbl:
        own = pf.unit_own_sites(d)
        if any(0 < n < pf.FLUSH_SITES for n in own):
            f.add("f32 unit with fewer than 64 own sites")
        if any(n > pf.FLUSH_SITES and n % pf.FLUSH_SITES for n in own):
            f.add("f32 unit whose own sites are no multiple of 64")
    if seg and 0 < d.W < d.L and d.n_units >= 2:
        r = d.W % df.UNIT_SITES
        f.add("W on a unit's first site" if r == 0 else "W on a unit's last site" if r == df.UNIT_SITES - 1 else "W inside a unit")
    return f


WANTED = ({f"K={K} {t}" for K in df.KS for t in ("f32", "f64")} | {f"L={L}" for L in df.LS}
          | {"nrm=1", "nrm=2", "nrm=4", "slab=particles", "slab=chunks", "inds permuted", "inds repeated", "inds subset",
             "per-chunk blocks differ", "W=L-1", "W=L", "het=0", "het=0.5", "miss=0.3", "missing runs", "raw method", "T=16 f64",
             "R_forward=16 at K=16 f32", "segmented, >= 3 units", "ragged lens with a row at W+1", "lens differ by row and by position",
             "row tiles under slab=particles", "row tiles under slab=chunks", "row tiles at nrm=1", "row tiles at nrm=2",
             "row tiles at nrm=4", "row tiles at T=16 f64", "f32 unit with fewer than 64 own sites", "f32 unit whose own sites are no multiple of 64",
             "W on a unit's first site", "W on a unit's last site", "W inside a unit"}
          | {"matrix path: " + x for x in ("serial", "segmented, >= 3 units", "T=8", "T=16", "nrm=1", "nrm=2", "nrm=4", "per-chunk blocks",
                                           "slab=particles", "slab=chunks")})


def test_default_seeds_cover_the_list():
    seen = set()
    for d in _defaults():
        seen |= _features(d)
    assert not WANTED - seen, f"the default seeds never draw: {sorted(WANTED - seen)}"


def test_streamed_oracle_is_the_dense_oracle():
    """``sequence_oracle`` sums xi_t site by site without keeping it: the same matrix as pair_count_oracle.pair_counts (another
    order of the float64 adds), the same ll."""
    import pair_count_oracle as pco

    d = _first(lambda d: d.Kc <= 16 and d.L - d.W >= 100 and d.lens is not None)
    o = pf.oracle(d)
    for b in range(d.B):
        for s in range(d.S):
            C, ll = pco.pair_counts(d.block(b, s), d.data[d.inds[s]], d.W, d.row_len(s))
            assert pco.error(o["seq"][b][s]["C"], C) < 1e-13 and o["ll"][b, s] == ll


def _first(pred):
    for d in _defaults():
        if pred(d):
            return d
    raise AssertionError("no default draw fits: change the draw")


def _swap_chunks(cand, d):  # two chunks' outputs swapped
    s0 = [s for s in range(d.S) if d.inds[s] != d.inds[0]][0]
    out = dict(cand, counts=cand["counts"].copy())
    out["counts"][:, [0, s0]] = out["counts"][:, [s0, 0]]
    return out


def test_comparators_catch_seeded_faults():
    """The oracle's own output passes on every default draw; with one fault injected it fails.  A float32 draw (the looser
    bars), ragged, with rows that differ, hets, a warm-up and a few hundred own sites in some rows."""
    for d in _defaults():
        ratio, msg, _ = pf.compare(pf.oracle(d), pf.oracle_candidate(d), d)
        assert ratio <= 1.0, (pf.describe(d), msg)

    d = _first(lambda d: not d.dbl and d.Kc <= 16 and d.K >= 8 and d.S >= 2 and len(np.unique(d.inds)) >= 2 and 0.0 < d.het < 0.5
               and d.W > 0 and d.lens is not None and any(int(d.lens[s]) != d.row_len(s) for s in range(d.S))
               and max(d.row_len(s) for s in range(d.S)) - d.W >= 200)
    o = pf.oracle(d)
    assert pf.compare(o, pf.pairs_candidate(d), d)[0] <= 1.0  # (the candidate builder itself, no fault)
    caught = []

    def check(name, cand, dd=d):
        ratio, msg, _ = pf.compare(pf.oracle(dd), cand, dd)
        print(f"pairs fault '{name}' on seed {dd.seed}: ratio {ratio:.3g} ({msg})")
        assert ratio > 1.0, name
        caught.append(name)

    def block(xi):  # one 8-site block's pair posteriors taken from its neighbour
        xi[96:104] = xi[104:112]
        return xi

    def dropped(xi):  # 64 consecutive sites never added (a float32 sum zeroed without going into the partial)
        xi[64:128] = 0.0
        return xi

    def tile(c, b, s):  # origin rows 4..7 zero: a row tile never added
        c = c.copy()
        c[4:8] = 0.0
        return c

    check("the matrix transposed", pf.pairs_candidate(d, matrix=lambda c, b, s: c.T))
    check("two chunks swapped", _swap_chunks(pf.oracle_candidate(d), d))
    check("lens by position", pf.pairs_candidate(d, row_len=lambda s: int(d.lens[s])))
    check("a site past a row's own length counted", pf.pairs_candidate(d, row_len=lambda s: min(d.row_len(s) + 1, d.L)))
    check("the last warm-up site counted", pf.pairs_candidate(d, W=d.W - 1))
    check("an 8-site block from its neighbour", pf.pairs_candidate(d, sites=block))
    check("64 consecutive sites dropped", pf.pairs_candidate(d, sites=dropped))
    check("rows 4..7 of the matrix zero", pf.pairs_candidate(d, matrix=tile))
    check("A applied twice", pf.pairs_candidate(d, matrix=lambda c, b, s: c * pn.dense_from_pp(d.block(b, s))))
    check("a float32 output", dict(pf.oracle_candidate(d), dtype="float32"))
    e = _first(lambda d: d.W == d.L)
    bad = pf.oracle_candidate(e)
    assert not bad["counts"].any() and not bad["ll"].any()
    bad["counts"][-1, -1, 0, 0] = 1e-300
    check("a non-zero entry at W = L", bad, e)
    assert len(caught) == 11


# ------------------------------------------------------------------------------------------------- GPU
STATS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if not STATS:
        return
    print("\npair fuzz summary (per float type)")
    for ft, rows in sorted(STATS.items()):
        w = max(rows, key=lambda r: r["ratio"])
        line = (f"  pairs {ft}: {len(rows)} draws, worst error/bar {w['ratio']:.3f} (seed {w['seed']}), worst counts error "
                f"{max(r.get('counts', 0.0) for r in rows):.3e}, worst |counts.sum() - own sites| {max(r.get('total', 0.0) for r in rows):.3e}")
        if ft == "f64":
            line += f", {sum(r['redrawn'] for r in rows)} of them float32 draws redrawn as float64"
        print(line)
    print(f"  wall time of test_pair_counts_random_shapes: {sum(r['time'] for rows in STATS.values() for r in rows):.1f} s (oracles included)")


def _call(d, kern, eng, pp, P, inds):
    """-> (ll, counts on the device; the candidate the comparator reads)"""
    import torch

    if d.raw:
        lens_t = None if d.lens is None else torch.as_tensor(d.lens, dtype=torch.int64).cuda()
        ll, c = eng.pair_counts(P, inds, d.W, lens=lens_t)
    else:
        ll, c = kern.pair_counts(pp, d.inds, lens=d.lens)
    assert ll.dtype == torch.float64
    return (ll, c), {"ll": ll.cpu().numpy(), "counts": c.cpu().numpy(), "dtype": str(c.dtype).replace("torch.", "")}


def _pair_draw(d, o, record=True, tag="pairs"):
    import torch

    t0 = time.perf_counter()
    kern, eng, pp, P, inds = tdf._setup(d)
    forced = d.plan is not None
    if forced:
        eng.set_plan(1 if d.plan[0] == "segmented" else 0, *d.plan[1:])
        ll0, g0 = eng.run(P, inds, d.W, grad=True)  # a gradient call before the sweep ...
        plan0 = eng.get_plan()
        if d.ws_limit is not None:  # (get_slab reports the last gradient call's slab, which counts checkpoints only)
            assert eng.get_slab() == d.grad_slab, (eng.get_slab(), d.grad_slab)

    def call():
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out = _call(d, kern, eng, pp, P, inds)
            risk = eng.underflow_risk()
        assert not risk, "underflow flag raised on ordinary parameters"
        return out

    a, cand = call()
    ratio, msg, info = pf.compare(o, cand, d)
    print(f"fuzz {tag} {pf.describe(d)}: counts {info.get('counts', float('nan')):.3e} |counts.sum() - own sites| "
          f"{info.get('total', float('nan')):.3e} worst error/bar {ratio:.3f}")
    assert ratio <= 1.0, msg
    b, _ = call()  # a repeat call: the same bits
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    if forced:
        ll1, g1 = eng.run(P, inds, d.W, grad=True)  # ... and after it: the same bits, the plan untouched
        assert torch.equal(ll0, ll1) and torch.equal(g0, g1)
        assert eng.get_plan() == plan0
    ll_post = eng.posterior(P, inds, d.W, bin=1)[0]  # the same legs at the same plan and W: ll to the bit
    assert torch.equal(a[0], ll_post), (a[0], ll_post)
    assert not eng.underflow_risk()
    if forced and d.ws_limit is not None:  # one launch instead of the slabs: the same bits (launch_pairs.hip)
        eng.set_workspace_limit(pf.LIFTED)
        c, _ = call()
        eng.set_workspace_limit(d.ws_limit)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), "bits differ between the slabs and one launch"
    if record:
        STATS.setdefault("f64" if d.dbl else "f32", []).append(
            dict(info, seed=d.seed, ratio=ratio, redrawn=d.redrawn, time=time.perf_counter() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_pair_counts_random_shapes(seed):
    d = pf.draw(seed)
    t0 = time.perf_counter()
    o = pf.oracle(d)
    t_oracle = time.perf_counter() - t0
    _pair_draw(d, o)
    STATS["f64" if d.dbl else "f32"][-1]["time"] += t_oracle


MANY_L, MANY_W, MANY_N = 48, 5, 4
MANY_SHAPES = [(3, 5), (4, 4), (17, 1), (9, 7), (8, 8), (13, 5)]  # B x S = 15, 16, 17, 63, 64, 65
_MANY: dict = {}


def _many(K):
    """-> (rows [4, 48], lens, a population of 17 models, the sequences' oracles shared between the shapes) for one K"""
    if K not in _MANY:
        rng = np.random.default_rng([31, K])
        rows = (rng.random((MANY_N, MANY_L)) < 0.1).astype(np.int8)
        rows[rng.random(rows.shape) < 0.05] = -1
        rows[:, 0] = 1
        pop = df._population(K, max(B for B, _ in MANY_SHAPES), seed=300 + K)
        _MANY[K] = (rows, np.array([48, 6, 29, 40]), pop, {})
    return _MANY[K]


@pytest.mark.gpu
@pytest.mark.parametrize("B,S", MANY_SHAPES)
@pytest.mark.parametrize("K", [16, 64])
def test_many_sequences(K, B, S):
    """float32, B x S just below, at and above what a wave (16 sequences at K = 16, 4 at K = 64) and a workgroup (64 and 16)
    hold: idle groups of lanes repeat the last sequence and must store nothing, every sequence is held to the comparator.  Rows
    of 48 sites with 5 of warm-up, 4 data rows behind repeated and permuted indices, ragged lens, one block per particle; a
    serial plan at T = 8 and a segmented one at T = 16."""
    rows, lens, pop, shared = _many(K)
    rng = np.random.default_rng([32, K, B, S])
    inds = rng.integers(0, MANY_N, size=S)
    if S > 1:
        inds[:2] = (3, 1)  # (permuted whatever else is drawn)
    pp = pn.PP(*(a[:B, None] for a in pop))
    R = K // 4
    for plan in (("serial", R, 8, R, 0), ("segmented", R, 16, R, R)):
        d = pf.manual_draw(K, False, rows, inds, pp, MANY_W, lens=lens, plan=plan, seed=1000 * K + 10 * B + S)
        _pair_draw(d, pf.oracle(d, shared), record=False, tag=f"many ({B} x {S})")


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
@pytest.mark.parametrize("M,pattern", [(16, "14*1+1*2"), (12, "10*1+1*2")])
def test_transition_counts_against_the_oracle(M, pattern, dbl):
    """``phlash_amd.transition_counts`` on two contigs of 137 and 60 windows (2 rows and 1 row) under two models.  ``per_model``
    is the sum of the rows' matrices: held, entry by entry on |x - ref| / max(1, ref), to the comparator's bar of one sequence
    whose own sites are all the rows' (the flat bar at scale max(1, 334 / 700) = 1; float32: 5 x the rows' summed E; float64: 5 x
    the rows' largest floor).  ``expected`` is linear in ``per_model``: expected[i, j] = mean over the models of
    rowsum_i(per_model) x A[i, j], so its absolute bar is the same map applied to the absolute bars of ``per_model``."""
    import torch

    import phlash_amd
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel

    rng = np.random.default_rng([33, M])
    contigs = [(rng.random((n, L)) < 0.03).astype(np.int8) for n, L in ((2, 137), (1, 60))]
    for c in contigs:
        c[rng.random(c.shape) < 0.02] = -1
        c[:, 0] = 1
    dm = DemographicModel.default(pattern, 1e-4, 1e-4)
    dms = [dm, DemographicModel(eta=dm.eta._replace(c=dm.eta.c * 1.5), theta=dm.theta, rho=dm.rho)]
    assert dm.M == M
    out = phlash_amd.transition_counts(dms, contigs, window_size=100, double_precision=dbl)
    # the oracle: the padded rows (missing windows past a contig's end) at their own lengths, the models per window
    data = np.full((3, 137), -1, np.int8)
    data[:2], data[2, :60] = contigs[0], contigs[1][0]
    per = [PSMCParams.from_dm(DemographicModel(eta=m.eta, theta=float(m.theta) * 100, rho=float(m.rho) * 100)) for m in dms]
    pp = pn.PP(*(np.stack([np.asarray(torch.as_tensor(getattr(p, f)).double().numpy(), float) for p in per])[:, None] for f in pn.PP._fields))
    d = pf.manual_draw(M, dbl, data, np.arange(3), pp, 0, lens=[137, 137, 60])
    o = pf.oracle(d)
    assert out.per_model.shape == (2, M, M) and out.per_model.dtype == torch.float64 and out.counts.shape == (M, M)
    got = out.per_model.cpu().numpy()
    n_own = sum(q["n_own"] for q in o["seq"][0])
    assert n_own == 334
    exp_ref, exp_bar = np.zeros((M, M)), np.zeros((M, M))
    for b in range(2):
        ref = sum(q["C"] for q in o["seq"][b])
        joint = {"C": ref, "n_own": n_own}
        if dbl:
            joint["floor"] = max(q["floor"] for q in o["seq"][b])
        else:
            joint["E"] = sum(q["E"] for q in o["seq"][b])
        bar = np.broadcast_to(pf.entry_bars(joint, dbl), ref.shape)
        err = np.abs(got[b] - ref) / np.maximum(1.0, ref)
        print(f"transition_counts M={M} {'f64' if dbl else 'f32'} model {b}: per_model error {err.max():.3e}, worst error/bar {(err / bar).max():.3f}")
        assert (err <= bar).all(), (b, float((err / bar).max()))
        A = pn.dense_from_pp(d.block(b, 0))
        exp_ref += ref.sum(1, keepdims=True) * A / 2
        exp_bar += (bar * np.maximum(1.0, ref)).sum(1, keepdims=True) * A / 2
    err = np.abs(out.expected.cpu().numpy() - exp_ref)
    print(f"transition_counts M={M} {'f64' if dbl else 'f32'}: expected error {err.max():.3e}, worst error/bar {(err / exp_bar).max():.3f}")
    assert (err <= exp_bar).all(), float((err / exp_bar).max())
    assert np.abs(out.counts.cpu().numpy() - got.mean(0)).max() <= 1e-12 * n_own


@pytest.mark.gpu
def test_regression_draws():
    """every pinned draw, whatever the number of seeds run (a loop: the table may be empty, and an empty parameter list skips)"""
    for name in sorted(REGRESSIONS):
        d = pf.draw(REGRESSIONS[name])
        _pair_draw(d, pf.oracle(d), record=False)
