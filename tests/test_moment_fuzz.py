"""Bin moments (phk_bin_moments) on seeded random draws (tests/moment_fuzz.py) against their float64 oracle.

CPU: what the bars need from the references alone (the float32 redraw share, the float32 emulation and the structured statement
inside their own bars), the coverage of the default seeds, and the comparator against the oracle's own output with one fault
injected.  GPU: one call per draw through ``PSMCKernel.bin_moments`` or the raw ``HipEngine`` method, held to the comparator, to
bitwise repeatability, to the gradient call's bits, plan and slab around it, to ``phk_posterior``'s ll and to the same bits with
the workspace limit lifted; more sequences than a wave and a workgroup hold.
``pytest -s -m gpu tests/test_moment_fuzz.py`` prints one ``fuzz`` line per draw and a summary (profiles/moment_fuzz.txt).
"""

from __future__ import annotations

import os
import time
import warnings

import numpy as np
import pytest

import decode_fuzz as df
import moment_bars as bars
import moment_fuzz as mf
import moment_oracle as mo
import test_decode_fuzz as tdf
from oracle import psmc_numpy as pn

DEFAULT_SEEDS = 64  # every item of test_default_seeds_cover_the_list is drawn within them
# draws that found a bug, kept by name whatever the number of seeds run: name -> seed
REGRESSIONS: dict = {}
N_SEEDS = int(os.environ.get("PHK_MOMENT_FUZZ_SEEDS", 64))


def _defaults():
    return [mf.draw(seed) for seed in range(DEFAULT_SEEDS)]


# ------------------------------------------------------------------------------------------------- CPU
def test_reference_alone_conditions():
    """The bars are derived from the references: this is where they are checked against the references, without a kernel.
    Float32 draws that float32 itself cannot hold are redrawn as float64 -- at most 5 % of them; the float32 emulation passes the
    comparator on every kept float32 draw and the structured statement on every float64 draw."""
    draws = _defaults()
    f32_default = [d for d in draws if not (d.seed // 10) % 2]
    redrawn = [d.seed for d in f32_default if d.redrawn]
    kept = [d for d in draws if not d.dbl]
    worst = max((mf.oracle(d)["redraw"] for d in kept), default=0.0)
    print(f"moments: {len(redrawn)} of {len(f32_default)} float32 draws redrawn as float64 (seeds {redrawn}); "
          f"largest 5 x E kept is {worst:.3f} of its cap")
    assert len(redrawn) <= 0.05 * len(f32_default), redrawn
    top, flat = (0.0, None), (0.0, None)
    for d in kept:
        o = mf.oracle(d)
        ratio, msg, _ = mf.compare(o, mf.oracle_candidate(d, "_32"), d)
        assert ratio <= 1.0, (mf.describe(d), msg)
        top = max(top, (ratio, d.seed))
        for row in o["seq"]:
            for q in row:
                if d.nbin:
                    e = np.maximum(mf.err(q["m1_32"], q["m1"]), mf.err(q["m2_32"], q["m2"])) / mf.scale_of(d, q["n_own"])
                    flat = max(flat, (float(e.max()), d.seed))
    print(f"moments: the float32 emulation on {len(kept)} float32 draws: worst ratio to its bars {top[0]:.3f} (seed {top[1]}); its "
          f"moments are at most {flat[0]:.3e} x scale off (seed {flat[1]}), {flat[0] / mf.F32_FLAT_BAR:.3f} of the flat bar, "
          f"{5 * flat[0] / df.F32_REDRAW_BAR:.3f} of the redraw cap")
    top, raw = (0.0, None), (0.0, None)
    n64 = 0
    for d in draws:
        if not d.dbl:
            continue
        n64 += 1
        o = mf.oracle(d)
        ratio, msg, _ = mf.compare(o, mf.oracle_candidate(d, "_s"), d)
        assert ratio <= 1.0, (mf.describe(d), msg)
        top = max(top, (ratio, d.seed))
        for row in o["seq"]:
            for q in row:
                if d.nbin:
                    e = np.maximum(mf.err(q["m1_s"], q["m1"]), mf.err(q["m2_s"], q["m2"])) / mf.scale_of(d, q["n_own"])
                    raw = max(raw, (float(e.max()) / bars.F64_MOMENT_BAR, d.seed))
    print(f"moments: the structured statement on {n64} float64 draws: worst ratio to its bars {top[0]:.3f} (seed {top[1]}); at most "
          f"{raw[0]:.3f} of F64_MOMENT_BAR x scale (seed {raw[1]})")


def _straddles(d):
    """a bin with sites in two units"""
    if not d.nbin:
        return False
    k = np.arange(d.nbin)
    return bool(((d.W + k * d.bin) // df.UNIT_SITES != d.bin_ends() // df.UNIT_SITES).any())


def _features(d):
    f = tdf._features(d)  # (the posterior draw's list; its values items never come up)
    if d.het == 0.5:
        f.add("het=0.5")
    if d.miss == 0.3:
        f.add("miss=0.3")
    if d.raw:
        f.add("raw method")
    if d.plan is not None and d.plan[2] == 16 and d.dbl:
        f.add("T=16 f64")
    n = d.L - d.W
    if d.lens is not None:
        own = [d.row_len(s) for s in range(d.S)]
        if len(set(own)) > 1 and d.W + 1 in own:
            f.add("ragged lens with a row at W+1")
        if any(d.lens[d.inds[s]] != d.lens[s] for s in range(d.S)):
            f.add("lens differ by row and by position")
        if any(x < d.L and (x - d.W) % d.bin for x in own):
            f.add("a row ends inside a bin")
    seg = mf.seg(d)
    if seg and 0 < d.W < d.L and d.n_units >= 2:
        r = d.W % df.UNIT_SITES
        f.add("W on a unit's first site" if r == 0 else "W on a unit's last site" if r == df.UNIT_SITES - 1 else "W inside a unit")
    f.add(f"values {d.form}")
    if d.v_rows and d.form != "zeros":
        assert all(not np.array_equal(d.vals[0], d.vals[b]) for b in range(1, d.B))
        if d.ws == "particles":
            f.add("[B,K] rows under slab=particles")
        if d.K != d.Kc:
            f.add("[B,K] rows at a padded K")
    if "per-chunk blocks differ" in f and not d.raw:
        f.add("per-chunk blocks through the API")
    if seg and d.bin > 2 * df.UNIT_SITES and n > 2 * df.UNIT_SITES and d.n_units >= 3:
        f.add("bin > 1024 under a segmented plan")
    if seg and d.n_units >= 2 and _straddles(d):
        f.add("bin straddles a unit edge")
    if d.bin == 1 and n >= 2:
        f.add("bin = 1")
    if d.nbin >= 2 and n % d.bin:
        f.add("last bin partial")
    return f


WANTED = ({f"K={K} {t}" for K in df.KS for t in ("f32", "f64")} | {f"L={L}" for L in df.LS} | {f"values {v}" for v in mf.FORMS}
          | {"nrm=1", "nrm=2", "nrm=4", "slab=particles", "slab=chunks", "inds permuted", "inds repeated", "inds subset",
             "per-chunk blocks differ", "W=L-1", "W=L", "het=0", "het=0.5", "miss=0.3", "missing runs", "raw method", "T=16 f64",
             "R_forward=16 at K=16 f32", "segmented, >= 3 units", "ragged lens with a row at W+1", "lens differ by row and by position",
             "W on a unit's first site", "W on a unit's last site", "W inside a unit",
             "[B,K] rows under slab=particles", "[B,K] rows at a padded K", "per-chunk blocks through the API",
             "bin > 512 under a segmented plan", "bin > 1024 under a segmented plan", "bin straddles a unit edge", "bin = 1",
             "last bin partial", "a row ends inside a bin"})


def test_default_seeds_cover_the_list():
    seen = set()
    for d in _defaults():
        seen |= _features(d)
    assert not WANTED - seen, f"the default seeds never draw: {sorted(WANTED - seen)}"


def _first(pred):
    for d in _defaults():
        if pred(d):
            return d
    raise AssertionError("no default draw fits: change the draw")


def _edit(cand, d, **arrays):
    """a candidate with m1 / m2 replaced (the API's mean and var follow them)"""
    return mf.finish(d, cand["ll"], arrays.get("m1", cand["m1"]), arrays.get("m2", cand["m2"]), mf.oracle(d)["maps"])


def _carry_right(d):
    """q1 and q2 not reset at a bin's last site: bin k holds the moments of S_k + S_{k+1}"""
    o, cand = mf.oracle(d), mf.oracle_candidate(d)
    m1, m2 = cand["m1"].copy(), cand["m2"].copy()
    for b in range(d.B):
        for s in range(d.S):
            for off in (0, 1):
                if d.W + off * d.bin >= d.L:
                    continue
                a1, a2, _ = mo.dense(d.block(b, s), d.data[d.inds[s]], o["maps"][b][2], d.W + off * d.bin, 2 * d.bin, d.row_len(s))
                for j in range(len(a1)):
                    if off + 2 * j < d.nbin - 1:
                        m1[b, s, off + 2 * j], m2[b, s, off + 2 * j] = a1[j], a2[j]
    return _edit(cand, d, m1=m1, m2=m2)


def _cut_at_unit_edge(d):
    """a bin that straddles a unit's edge holds the sites right of the edge only"""
    o, cand = mf.oracle(d), mf.oracle_candidate(d)
    k = [k for k in range(d.nbin) if (d.W + k * d.bin) // df.UNIT_SITES != d.bin_ends()[k] // df.UNIT_SITES][0]
    end = int(d.bin_ends()[k])
    edge = end // df.UNIT_SITES * df.UNIT_SITES
    m1, m2 = cand["m1"].copy(), cand["m2"].copy()
    for b in range(d.B):
        for s in range(d.S):
            a1, a2, _ = mo.dense(d.block(b, s), d.data[d.inds[s], : end + 1], o["maps"][b][2], edge, end - edge + 1, d.row_len(s))
            m1[b, s, k], m2[b, s, k] = a1[0], a2[0]
    return _edit(cand, d, m1=m1, m2=m2)


def test_comparators_catch_seeded_faults():
    """The oracle's own output passes on every default draw; with one fault injected it fails.  A float32 draw (the looser
    bars), ragged, with a warm-up, rows that differ and a value row per particle."""
    for d in _defaults():
        ratio, msg, _ = mf.compare(mf.oracle(d), mf.oracle_candidate(d), d)
        assert ratio <= 1.0, (mf.describe(d), msg)

    d = _first(lambda d: not d.dbl and d.S >= 2 and len(np.unique(d.inds)) >= 2 and d.W > 0 and d.lens is not None and d.v_rows
               and not mf.flat(d) and any(int(d.lens[s]) != d.row_len(s) for s in range(d.S)) and d.nbin >= 3 and d.bin >= 2
               and max(d.row_len(s) for s in range(d.S)) - d.W >= 3 * d.bin)
    o = mf.oracle(d)
    good = mf.oracle_candidate(d)
    assert mf.compare(o, mf.moments_candidate(d), d)[0] <= 1.0  # (the candidate builder itself, no fault)
    caught = []

    def check(name, cand, dd=d):
        ratio, msg, _ = mf.compare(mf.oracle(dd), cand, dd)
        print(f"moments fault '{name}' on seed {dd.seed}: ratio {ratio:.3g} ({msg})")
        assert ratio > 1.0, name
        caught.append(name)

    def independent(q, b, s):  # m1^2 plus the sites' variances: no covariance between the sites of a bin
        return q["m1"] ** 2 + mf.site_sums(q["m2_site"] - q["m1_site"] ** 2, d.bin, len(q["m1"]))

    def swap_chunks(cand, dd):
        s0 = [s for s in range(dd.S) if dd.inds[s] != dd.inds[0]][0]
        m1, m2 = cand["m1"].copy(), cand["m2"].copy()
        m1[:, [0, s0]], m2[:, [0, s0]] = m1[:, [s0, 0]], m2[:, [s0, 0]]
        return _edit(cand, dd, m1=m1, m2=m2)

    check("another particle's value row", mf.moments_candidate(d, values=lambda b: o["maps"][(b + 1) % d.B][2]))
    check("lens by position", mf.moments_candidate(d, row_len=lambda s: int(d.lens[s])))
    check("a site past a row's own length counted", mf.moments_candidate(d, row_len=lambda s: min(d.row_len(s) + 1, d.L)))
    check("the last warm-up site counted", mf.moments_candidate(d, W=d.W - 1))
    check("bins shifted one site", mf.moments_candidate(d, shift=1))
    check("q1 and q2 not reset at a bin's last site", _carry_right(d))
    check("m2 without the cross term", mf.moments_candidate(d, m2=independent))
    check("m1 and m2 swapped", _edit(good, d, m1=good["m2"], m2=good["m1"]))
    check("two chunks swapped", swap_chunks(good, d))
    check("a float32 output", dict(good, dtype="float32"))
    e = _first(lambda d: mf.seg(d) and d.n_units >= 2 and _straddles(d) and not mf.flat(d) and not d.dbl)
    check("a bin cut at a unit's edge", _cut_at_unit_edge(e), e)
    e = _first(lambda d: not d.raw and d.B >= 2 and not mf.flat(d) and d.nbin >= 1 and not d.dbl)
    shifted = [mf.centre(e, b, pi_of=0) for b in range(e.B)]  # (mean and var are mapped back with the same centre: only m1 and m2 tell)
    check("the centre under particle 0's pi for every particle", mf.moments_candidate(e, values=lambda b: shifted[b][2], maps=shifted), e)
    e = _first(lambda d: d.lens is not None and any(d.row_len(s) - d.W <= (d.nbin - 1) * d.bin for s in range(d.S)))
    bad = mf.oracle_candidate(e)
    s = [s for s in range(e.S) if e.row_len(s) - e.W <= (e.nbin - 1) * e.bin][0]
    assert bad["m1"][0, s, -1] == 0.0
    bad["m1"][0, s, -1] = 1e-300
    check("1e-300 in a bin without a site of the row's own", bad, e)
    e = _first(lambda d: d.W == d.L)
    bad = mf.oracle_candidate(e)
    assert not bad["ll"].any() and bad["m1"].size == 0
    bad["ll"][-1, -1] = 1e-300
    check("a non-zero ll at W = L", bad, e)
    assert len(caught) == 14


def test_moments32_is_the_dense_oracle_in_float32():
    """the emulation against the oracle on one short sequence: float32 close, and its bins and masking the oracle's"""
    d = _first(lambda d: not d.dbl and d.lens is not None and not mf.flat(d) and d.nbin >= 2)
    q = mf.oracle(d)["seq"][0][0]
    assert q["m1_32"].shape == q["m1"].shape and (q["m1_32"] == 0).tolist() == (q["m1"] == 0).tolist()
    assert float(np.maximum(mf.err(q["m1_32"], q["m1"]), mf.err(q["m2_32"], q["m2"])).max()) < 1e-3


# ------------------------------------------------------------------------------------------------- GPU
STATS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if not STATS:
        return
    print("\nmoment fuzz summary (per float type)")
    for ft, rows in sorted(STATS.items()):
        w = max(rows, key=lambda r: r["ratio"])
        line = (f"  moments {ft}: {len(rows)} draws, worst error/bar {w['ratio']:.3f} (seed {w['seed']}), worst m1 error "
                f"{max(r.get('m1', 0.0) for r in rows):.3e}, worst m2 error {max(r.get('m2', 0.0) for r in rows):.3e}")
        if ft == "f64":
            line += f", {sum(r['redrawn'] for r in rows)} of them float32 draws redrawn as float64"
        print(line)
    print(f"  wall time of test_bin_moments_random_shapes: {sum(r['time'] for rows in STATS.values() for r in rows):.1f} s (oracles included)")


def _call(d, kern, eng, pp, P, inds):
    """-> (the call's device tensors; the candidate the comparator reads)"""
    import torch

    if d.raw:
        lens_t = None if d.lens is None else torch.as_tensor(d.lens, dtype=torch.int64).cuda()
        out = eng.bin_moments(P, inds, torch.as_tensor(d.vals, dtype=torch.float64).cuda(), d.W, bin=d.bin, lens=lens_t)
        named = dict(zip(("ll", "m1", "m2"), out))
    else:
        out = kern.bin_moments(pp, d.inds, values=d.vals, bin=d.bin, lens=d.lens)
        named = out._asdict()
    types = {str(x.dtype).replace("torch.", "") for x in out}
    cand = {k: x.cpu().numpy() for k, x in named.items()}
    cand["dtype"] = types.pop() if len(types) == 1 else str(sorted(types))
    return tuple(out), cand


def _moment_draw(d, o, record=True, tag="moments"):
    import torch

    t0 = time.perf_counter()
    kern, eng, pp, P, inds = tdf._setup(d)
    forced = d.plan is not None
    if forced:
        eng.set_plan(1 if d.plan[0] == "segmented" else 0, *d.plan[1:])
        ll0, g0 = eng.run(P, inds, d.W, grad=True)  # a gradient call before the sweep ...
        plan0 = eng.get_plan()
        if d.ws_limit is not None:  # (no workspace of the sweep's own: the gradient call's slab is the sweep's)
            assert eng.get_slab() == d.slab, (eng.get_slab(), d.slab)

    def call():
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            out = _call(d, kern, eng, pp, P, inds)
            risk = eng.underflow_risk()
        assert not risk, "underflow flag raised on ordinary parameters"
        return out

    a, cand = call()
    ratio, msg, info = mf.compare(o, cand, d)
    print(f"fuzz {tag} {mf.describe(d)}: nbin={d.nbin} m1 {info.get('m1', float('nan')):.3e} m2 {info.get('m2', float('nan')):.3e} "
          f"worst error/bar {ratio:.3f}")
    assert ratio <= 1.0, msg
    b, _ = call()  # a repeat call: the same bits
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    if forced:
        ll1, g1 = eng.run(P, inds, d.W, grad=True)  # ... and after it: the same bits, the plan untouched
        assert torch.equal(ll0, ll1) and torch.equal(g0, g1)
        assert eng.get_plan() == plan0
        if d.ws_limit is not None:
            assert eng.get_slab() == d.slab, (eng.get_slab(), d.slab)
    ll_post = eng.posterior(P, inds, d.W, bin=d.bin)[0]  # the same legs at the same plan, W and bin: ll to the bit
    assert torch.equal(a[0], ll_post), (a[0], ll_post)
    assert not eng.underflow_risk()
    if forced and d.ws_limit is not None:  # one launch instead of the slabs: the same bits
        eng.set_workspace_limit(mf.LIFTED)
        c, _ = call()
        eng.set_workspace_limit(d.ws_limit)
        assert all(torch.equal(x, y) for x, y in zip(a, c)), "bits differ between the slabs and one launch"
    if record:
        STATS.setdefault("f64" if d.dbl else "f32", []).append(
            dict(info, seed=d.seed, ratio=ratio, redrawn=d.redrawn, time=time.perf_counter() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_bin_moments_random_shapes(seed):
    d = mf.draw(seed)
    t0 = time.perf_counter()
    o = mf.oracle(d)
    t_oracle = time.perf_counter() - t0
    _moment_draw(d, o)
    STATS["f64" if d.dbl else "f32"][-1]["time"] += t_oracle


MANY_L, MANY_W, MANY_N, MANY_BIN = 48, 5, 4, 5
MANY_SHAPES = [(3, 5), (4, 4), (17, 1), (9, 7), (8, 8), (13, 5)]  # B x S = 15, 16, 17, 63, 64, 65
_MANY: dict = {}


def _many(K):
    """-> (rows [4, 48], lens, a population of 17 models, a value row and a map into other units per model, the sequences'
    oracles shared between the shapes) for one K"""
    if K not in _MANY:
        rng = np.random.default_rng([41, K])
        rows = (rng.random((MANY_N, MANY_L)) < 0.1).astype(np.int8)
        rows[rng.random(rows.shape) < 0.05] = -1
        rows[:, 0] = 1
        nB = max(B for B, _ in MANY_SHAPES)
        pop = df._population(K, nB, seed=400 + K)
        c = 10.0 ** rng.uniform(-2.0, 3.0, size=nB)
        _MANY[K] = (rows, np.array([48, 6, 29, 40]), pop, rng.uniform(-1.0, 1.0, (nB, K)), c * rng.uniform(-3.0, 3.0, size=nB), c, {})
    return _MANY[K]


@pytest.mark.gpu
@pytest.mark.parametrize("B,S", MANY_SHAPES)
@pytest.mark.parametrize("K", [16, 64])
def test_many_sequences(K, B, S):
    """float32, B x S just below, at and above what a wave (16 sequences at K = 16, 4 at K = 64) and a workgroup (64 and 16)
    hold: idle groups of lanes repeat the last sequence and must store nothing, every sequence is held to the comparator.  Rows
    of 48 sites with 5 of warm-up in bins of 5, 4 data rows behind repeated and permuted indices, ragged lens, one block and
    one signed value row per particle, through the API; a serial plan at T = 8 and a segmented one at T = 16."""
    rows, lens, pop, vals, a, c, shared = _many(K)
    rng = np.random.default_rng([42, K, B, S])
    inds = rng.integers(0, MANY_N, size=S)
    if S > 1:
        inds[:2] = (3, 1)  # (permuted whatever else is drawn)
    pp = pn.PP(*(x[:B, None] for x in pop))
    R = K // 4
    for plan in (("serial", R, 8, R, 0), ("segmented", R, 16, R, R)):
        d = mf.manual_draw(K, False, rows, inds, pp, MANY_W, vals[:B], MANY_BIN, lens=lens, plan=plan, seed=1000 * K + 10 * B + S,
                           map_a=a[:B], map_c=c[:B])
        _moment_draw(d, mf.oracle(d, shared), record=False, tag=f"many ({B} x {S})")


@pytest.mark.gpu
def test_regression_draws():
    """every pinned draw, whatever the number of seeds run (a loop: the table may be empty, and an empty parameter list skips)"""
    for name in sorted(REGRESSIONS):
        d = mf.draw(REGRESSIONS[name])
        _moment_draw(d, mf.oracle(d), record=False)
