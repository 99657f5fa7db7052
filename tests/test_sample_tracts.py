"""Sampled tract spectra (phk_sample_tracts, PSMCKernel.sample_tracts, path_tracts, tract_lengths): the paths of posterior path
sampling reduced inside the kernel to tract counts, a length histogram and the cover of long tracts.

Everything here is integer, so every comparison is exact equality:
* ``path_tracts`` (vectorised torch, the product's statement of the definition) against a site-by-site Python loop;
* the float64 kernel against ``path_tracts`` of the ORACLE's paths (tests/sampling_oracle.py) on the sampling grid, whose margin
  condition test_path_sampling asserts;
* both float types against ``path_tracts`` of the paths ``sample_paths`` stores on the same handle, seed and plan.
The statistical anchors (independent of phk_sample_paths) use the project's bar of 6 standard errors.  The standard error comes
from the across-sample variance, floored at the variance of one sample in N differing by one site (1 / N): a count on which
every sample agrees would otherwise have none.  ``cover`` is a sum over the samples, so its per-sample variance is taken from
the oracle's draws on the same input (the float64 kernel makes exactly those draws).
"""

from __future__ import annotations

import functools
import warnings

import numpy as np
import pytest
import torch

import posterior_oracle as po
import sampling_oracle as so
from test_path_sampling import (EDGE_B, EDGE_K, EDGE_L, EDGE_S, GRID_SAMPLES, GRID_SEED, GRID_W, MIN_MARGIN, STAT_N, STAT_SEED, _params,
                                edge_rows, grid_reference, stat_inputs)
from test_viterbi import GRID_K, _bcast, _per_chunk, _population, _rows, grid_inputs

GRID_EDGES, GRID_BIN, GRID_MIN_LEN = (2, 5, 20), 7, 3
EDGES15 = tuple(range(1, 16))
STAT_BIN = 8
SE_BAR = 6.0


def younger_states(K):
    """the tests' set: the younger three quarters of the states.  The posterior paths of the sampling grid live in the upper
    half of the states, and this cut splits their mass about 1 : 2 for K >= 8 (at K = 4 every path sits in state 2: one tract)"""
    return np.arange(K) < 3 * K // 4


# ------------------------------------------------------------------------------------------------- the plain statement
def loop_tracts(paths, in_set, edges=(), lens=None, min_len=1, bin=None):
    """The definition, site by site.  paths [..., n, L] integers; in_set bool [M] or [B, M] (B: the first dimension of paths);
    lens: own reported sites, broadcastable to paths.shape[:-2].  -> (counts [..., n, 4], hist [..., n, C], cover [..., nbin] or None)"""
    paths = np.asarray(paths)
    in_set = np.asarray(in_set, bool)
    lead, n, L = paths.shape[:-2], paths.shape[-2], paths.shape[-1]
    C = len(edges) + 1
    own = np.broadcast_to(np.full(lead, L) if lens is None else np.asarray(lens), lead)
    counts = np.zeros(lead + (n, 4), np.int64)
    hist = np.zeros(lead + (n, C), np.int64)
    nbin = None if bin is None else (L + bin - 1) // bin
    cover = None if bin is None else np.zeros(lead + (nbin,), np.int64)
    for idx in np.ndindex(*lead):
        member = in_set if in_set.ndim == 1 else in_set[idx[0]]
        ln = int(min(max(own[idx], 0), L))
        for r in range(n):
            z = paths[idx + (r,)]
            c = counts[idx + (r,)]
            run = 0
            for t in range(ln + 1):  # (t = ln: the end of the row closes an open tract)
                inside = t < ln and int(z[t]) < len(member) and bool(member[int(z[t])])
                if 0 < t < ln and z[t] != z[t - 1]:
                    c[3] += 1
                if inside:
                    c[0] += 1
                    run += 1
                elif run > 0:
                    c[1] += 1
                    c[2] = max(c[2], run)
                    hist[idx + (r, sum(1 for e in edges if e <= run))] += 1
                    if bin is not None and run >= min_len:
                        for u in range(t - run, t):
                            cover[idx + (u // bin,)] += 1
                    run = 0
    return counts, hist, cover


def mismatches(a, b):
    """the comparator: entries at which two (counts, hist, cover) triples differ (a shape mismatch counts everything)"""
    total = 0
    for x, y in zip(a, b):
        if x is None and y is None:
            continue
        x, y = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x), np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y)
        total += int((x != y).sum()) if x.shape == y.shape else max(x.size, y.size)
    return total


def _pt(paths, in_set, **kw):
    from phlash_amd import path_tracts

    return path_tracts(torch.as_tensor(np.asarray(paths)) if not isinstance(paths, torch.Tensor) else paths, in_set, **kw)


# ------------------------------------------------------------------------------------------------- shared references
@functools.lru_cache(maxsize=None)
def grid_expected(K):
    """{(W, layout): (PathTracts of the float64 ORACLE's paths [2, S, n, 700 - W], ll [2, S])} on the sampling grid: computed once,
    shared with the GPU test (read only)"""
    out = {}
    for key, (paths, _, ll) in grid_reference(K).items():
        stacked = np.stack([np.stack(ps) for ps in paths])
        out[key] = (_pt(stacked, younger_states(K), edges=GRID_EDGES, min_len=GRID_MIN_LEN, bin=GRID_BIN), ll)
    return out


@functools.lru_cache(maxsize=None)
def stat_reference(bits24=False):
    """the statistical input (K = 8, one row of 96 windows, 4,096 draws) under the oracle: expected values from the exact
    posteriors, the oracle's own draws reduced by path_tracts, and the per-sample standard deviation of the per-bin counts"""
    pp, row, gamma, _ = stat_inputs()
    member = younger_states(8)
    paths, _ = so.sample(pp, row, 0, q=0, n_samples=STAT_N, seed=STAT_SEED, bits24=bits24)
    marg = gamma[:, member].sum(1)  # P(z_t in the set | o)
    changes = sum(1.0 - float(np.trace(so.pair_posterior(pp, row, t))) for t in range(len(row) - 1))
    res = _pt(paths, member, min_len=1, bin=STAT_BIN)
    per_bin = member[paths.astype(int)].reshape(STAT_N, -1, STAT_BIN).sum(2)  # [N, nbin]
    return dict(inside=float(marg.sum()), changes=changes, bins=marg.reshape(-1, STAT_BIN).sum(1), res=res, bin_sd=per_bin.std(0))


def se_score(values, expect):
    """|mean - expect| in standard errors of the mean of ``values`` (variance floored at 1 / N)"""
    v = np.asarray(values, float)
    return float(abs(v.mean() - expect) / np.sqrt(max(v.var(), 1.0 / len(v)) / len(v)))


def cover_scores(cover, n, expect_bins, bin_sd):
    return np.abs(np.asarray(cover, float) / n - expect_bins) / np.sqrt(np.maximum(bin_sd ** 2, 1.0 / n) / n)


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K", [2, 4, 16, 64])
@pytest.mark.parametrize("L", [1, 2, 17, 130])
def test_path_tracts_equals_the_plain_loop(K, L):
    rng = np.random.default_rng(1000 * K + L)
    B, S, n = 2, 3, 2
    # sticky paths, so that tracts are longer than a site or two
    steps = rng.random((B, S, n, L)) < 0.3
    fresh = rng.integers(0, K, size=(B, S, n, L))
    paths = np.empty((B, S, n, L), np.uint8)
    paths[..., 0] = fresh[..., 0]
    for t in range(1, L):
        paths[..., t] = np.where(steps[..., t], fresh[..., t], paths[..., t - 1])
    one = np.zeros(K, bool)
    one[K // 2] = True
    per_particle = rng.random((B, K)) < 0.5
    masks = [np.zeros(K, bool), np.ones(K, bool), one, rng.random(K) < 0.5, per_particle]
    lens_options = [None, np.array([1, L, max(1, L // 2)])]  # (1: a single reported site, len = W + 1 in a call's terms)
    combos = [((), 1, 1), (EDGES15, 7, 5), (EDGES15, 64, L + 1), ((), L + 3, 1), (EDGES15, 1, 5), ((3,), 7, 1), (EDGES15, None, 1)]
    on_edge = False
    for member in masks:
        for lens in lens_options:
            for edges, bin, min_len in combos:
                want = loop_tracts(paths, member, edges, lens, min_len, bin)
                got = _pt(paths, member, edges=edges, lens=lens, min_len=min_len, bin=bin)
                assert got.counts.dtype == torch.int32 and got.counts.shape == (B, S, n, 4) and got.hist.shape == (B, S, n, len(edges) + 1)
                assert (got.cover is None) == (bin is None)
                assert mismatches(got, want) == 0, (K, L, member, lens, edges, bin, min_len)
                if edges == EDGES15:
                    on_edge = on_edge or bool(want[1][..., 1:].sum() > 0)  # (classes 1 .. 15 hold lengths >= an edge)
    if L >= 17:
        assert on_edge, "no tract length on an edge: the upper-class rule went untested"


def test_path_tracts_on_hand_written_paths():
    m = np.array([True, False, False])  # state 0 is inside
    # 12 sites, bins of 4.  Tracts: [0, 2) touches the first site; [5, 7) inside bin 1; [9, 12) ends at the last site
    p = np.array([[[0, 0, 1, 2, 2, 0, 0, 1, 1, 0, 0, 0]]])
    r = _pt(p, m, edges=(2, 3), min_len=1, bin=4)
    assert r.counts.tolist() == [[[7, 3, 3, 5]]]
    assert r.hist.tolist() == [[[0, 2, 1]]]  # lengths 2, 2 (on the edge 2: upper class) and 3 (on the edge 3)
    assert r.cover.tolist() == [[2, 2, 3]]
    assert _pt(p, m, edges=(2, 3), min_len=3, bin=4).cover.tolist() == [[0, 0, 3]]
    # a tract over whole bins with a partial first and last bin: sites 2 .. 9 of 12, bins of 3 -> 1, 3, 3, 1
    p = np.array([[[1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2]]])
    r = _pt(p, m, edges=(8,), min_len=8, bin=3)
    assert r.counts.tolist() == [[[8, 1, 8, 2]]] and r.hist.tolist() == [[[0, 1]]] and r.cover.tolist() == [[1, 3, 3, 1]]
    assert _pt(p, m, min_len=9, bin=3).cover.tolist() == [[0, 0, 0, 0]]
    # two tracts in one bin, the shorter one below min_len; two samples add up in cover
    p = np.array([[[0, 1, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0]]])
    r = _pt(p, m, edges=(2,), min_len=2, bin=6)
    assert r.counts.tolist() == [[[3, 2, 2, 3], [6, 1, 6, 0]]] and r.hist.tolist() == [[[1, 1], [0, 1]]] and r.cover.tolist() == [[2 + 6]]
    # the row's own length: the tract that reaches it ends there, at its visible length; pairs behind it do not count
    p = np.array([[[1, 0, 0, 0, 0, 2]]])
    r = _pt(p, m, lens=np.array([3]), edges=(2, 4), bin=2)
    assert r.counts.tolist() == [[[2, 1, 2, 1]]] and r.hist.tolist() == [[[0, 1, 0]]] and r.cover.tolist() == [[1, 1, 0]]
    # one set per particle; a 255 (past a Viterbi row's end) is outside every set
    p = np.array([[[[0, 0, 1, 255]]], [[[0, 0, 1, 255]]]], dtype=np.uint8)
    r = _pt(p, np.array([[True, False], [False, True]]))
    assert r.counts[..., :3].tolist() == [[[[2, 1, 2]]], [[[1, 1, 1]]]]


def test_comparator_fails_on_injected_faults():
    rng = np.random.default_rng(4)
    paths = np.repeat(rng.integers(0, 4, size=(2, 3, 20)), 5, axis=-1).astype(np.uint8)  # [2, 3 samples, 100]: runs of 5
    m = np.array([True, True, False, False])
    kw = dict(edges=(5, 10), min_len=5, bin=7)
    want = loop_tracts(paths, m, **kw)
    assert mismatches(_pt(paths, m, **kw), want) == 0
    assert mismatches(_pt(np.roll(paths, 1, axis=-1), m, **kw), want) > 0  # sites shifted by one
    swapped = paths.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]
    sw = _pt(swapped, m, **kw)
    assert mismatches(sw, want) > 0 and mismatches((sw.cover,), (want[2],)) == 0  # samples swapped: cover, a sum over them, cannot tell
    off = _pt(paths, m, edges=(6, 11), min_len=5, bin=7)  # a length on an edge sent to the lower class
    assert mismatches((off.hist,), (want[1],)) > 0 and mismatches((off.counts, off.cover), (want[0], want[2])) == 0


def test_phk_sample_tracts_rejects_bad_arguments_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_sample_tracts" in _lib.SIGNATURES
    rc = lib.phk_sample_tracts(None, None, 0, 0, None, None, 1, 1, 0, 1, 0, None, 0, None, None, 0, 1, 1, None, None, None, None)
    assert rc == _lib.PHK_EINVAL
    assert lib.phk_last_error() == b"handle is NULL"
    rc = lib.phk_sample_paths(None, None, 0, 0, None, None, 1, 1, 0, 1, 0, None, None, 0, None)
    assert rc == _lib.PHK_EINVAL and lib.phk_last_error() == b"handle is NULL"  # word for word phk_sample_paths'


def test_tract_lengths_is_lazy_and_has_no_cpu_fallback(monkeypatch):
    import phlash_amd
    from phlash_amd.decode import path_tracts, tract_lengths
    from phlash_amd.kernel import PSMCKernel, TractSample

    assert phlash_amd.tract_lengths is tract_lengths and phlash_amd.path_tracts is path_tracts
    assert phlash_amd.TractLengths._fields == ("spectrum", "n_tracts", "longest", "inside", "in_long", "counts", "hist")
    assert hasattr(PSMCKernel, "sample_tracts") and TractSample._fields == ("ll", "counts", "hist", "cover")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dm = phlash_amd.DemographicModel.default("4*1", 1e-4, 1e-4)
    data = np.zeros((1, 50), dtype=np.int8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        tract_lengths(dm, data, t_max=1.0)


@pytest.mark.parametrize("K", GRID_K)
def test_expected_answers_of_the_gpu_grid(K):
    exp = grid_expected(K)
    assert set(exp) == {(W, layout) for W in GRID_W for layout in ("bcast", "chunk")}
    paths = grid_reference(K)[GRID_W[1], "chunk"][0]
    for (W, layout), (res, ll) in exp.items():
        n = 700 - W
        assert res.counts.shape == (2, 3, GRID_SAMPLES, 4) and res.hist.shape == (2, 3, GRID_SAMPLES, 4) and res.cover.shape == (2, 3, (n + 6) // 7)
        assert torch.equal(res.hist.sum(-1), res.counts[..., 1]) and int(res.counts[..., 0].max()) <= n
        assert int(res.counts[..., 1].sum()) > 0, "a grid without a tract tests little"
    # one sequence against the plain loop
    res = exp[GRID_W[1], "chunk"][0]
    want = loop_tracts(paths[1][2], younger_states(K), GRID_EDGES, None, GRID_MIN_LEN, GRID_BIN)
    assert mismatches((res.counts[1, 2], res.hist[1, 2], res.cover[1, 2]), want) == 0


@pytest.mark.parametrize("bits24", [False, True])
def test_statistical_scores_on_the_oracle_draws(bits24):
    ref = stat_reference(bits24)
    c = ref["res"].counts.numpy()
    inside, changes = se_score(c[:, 0], ref["inside"]), se_score(c[:, 3], ref["changes"])
    cov = cover_scores(ref["res"].cover.numpy(), STAT_N, ref["bins"], ref["bin_sd"])
    print(f"STAT tracts oracle {'24-bit' if bits24 else '53-bit'} uniforms: inside {inside:.2f}, changes {changes:.2f}, worst bin of cover "
          f"{cov.max():.2f} standard errors (the bar is {SE_BAR:g})")
    assert inside < SE_BAR and changes < SE_BAR and cov.max() < SE_BAR
    # at min_len = 1 every site inside the set lies in a counted tract: cover sums to column 0
    assert int(ref["res"].cover.sum()) == int(c[:, 0].sum())


# ------------------------------------------------------------------------------------------------- GPU
def _mask_words(in_set):
    m = np.atleast_2d(np.asarray(in_set, bool))
    words = [sum(1 << k for k in range(m.shape[1]) if row[k]) for row in m]
    return torch.tensor([w - (1 << 64) if w >= 1 << 63 else w for w in words], dtype=torch.int64, device="cuda")


def _triple(out):
    return (out.counts, out.hist, out.cover)


def _stats_triple(stats, cover):
    return (stats[..., :4], stats[..., 4:], cover)


@pytest.mark.gpu
@pytest.mark.parametrize("K", GRID_K)
def test_f64_equals_path_tracts_of_the_oracle_paths(K):
    from phlash_amd.kernel import get_kernel

    pp, pc, sets = grid_inputs(K)
    exp, ref = grid_expected(K), grid_reference(K)
    worst = 0.0
    for (rows, _, _), W in zip(sets, GRID_W):
        S = len(rows)
        kern = get_kernel(K, rows, double_precision=True, overlap=W)
        for layout in ("bcast", "chunk"):
            assert min(float(m.min()) for ms in ref[W, layout][1] for m in ms) >= MIN_MARGIN
            q = _bcast(pp) if layout == "bcast" else _per_chunk(pc, S)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                out = kern.sample_tracts(q, np.arange(S), in_set=younger_states(K), n_samples=GRID_SAMPLES, seed=GRID_SEED, edges=GRID_EDGES,
                                         min_len=GRID_MIN_LEN, bin=GRID_BIN)
            want, rll = exp[W, layout]
            assert out.counts.dtype == torch.int32 and out.cover.dtype == torch.int32
            bad = mismatches(_triple(out), want)
            assert bad == 0, f"K={K} W={W} {layout}: {bad} entries of stats / cover differ from path_tracts of the oracle's paths"
            worst = max(worst, float(np.abs(out.ll.cpu().numpy() / rll - 1).max()))
    print(f"PARITY tracts K={K} f64: stats and cover equal the oracle's at every entry; max rel ll error {worst:.3e}")
    assert worst < 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [True, False])
@pytest.mark.parametrize("K", GRID_K)
def test_both_types_equal_path_tracts_of_their_own_stored_paths(K, dbl):
    from phlash_amd.kernel import get_kernel

    pp, pc, sets = grid_inputs(K)
    for (rows, _, _), W in zip(sets, GRID_W):
        S = len(rows)
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        for layout in ("bcast", "chunk"):
            q = _bcast(pp) if layout == "bcast" else _per_chunk(pc, S)
            kw = dict(n_samples=GRID_SAMPLES, seed=GRID_SEED)
            out = kern.sample_tracts(q, np.arange(S), in_set=younger_states(K), edges=GRID_EDGES, min_len=GRID_MIN_LEN, bin=GRID_BIN, **kw)
            stored = kern.sample_paths(q, np.arange(S), **kw)
            want = _pt(stored.paths, younger_states(K), edges=GRID_EDGES, min_len=GRID_MIN_LEN, bin=GRID_BIN)
            assert mismatches(_triple(out), want) == 0, (K, dbl, W, layout)
            assert torch.equal(out.ll, stored.ll), (K, dbl, W, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [True, False])
def test_block_and_unit_edges(dbl):
    from phlash_amd.engine import HipEngine

    P = _params(_population(EDGE_K, EDGE_B, seed=11))
    inds = torch.arange(EDGE_S, device="cuda")
    member = younger_states(EDGE_K)
    masks = _mask_words(member)
    plans = [(0, 4, 8, 4, 0), (0, 4, 16, 4, 0)] + ([] if dbl else [(0, 4, 8, 16, 0)])  # the last: one state per lane forward kernel
    for L in EDGE_L:
        eng = HipEngine(EDGE_K, edge_rows(L), double_precision=dbl)
        for W in sorted({0, L - 1}):
            # own lengths: full and a single reported site (len = W + 1); on a block boundary and inside a block
            lens_options = [None, [W + 1, L]] + ([[min(L, 16), min(L, 21)], [min(L, 8), min(L, 13)]] if W == 0 and L > 1 else [])
            for plan in plans:
                eng.set_plan(*plan)
                for lens in lens_options:
                    lt = None if lens is None else torch.tensor(lens, dtype=torch.int64, device="cuda")
                    kw = dict(warmup=W, n_samples=3, seed=4321)
                    ll, stats, cover = eng.sample_tracts(P, inds, masks, edges=(2, 4, 9), lens=lt, min_len=2, bin=5, **kw)
                    ll2, paths = eng.sample_paths(P, inds, **kw)
                    assert not eng.underflow_risk()
                    want = _pt(paths, member, edges=(2, 4, 9), lens=None if lens is None else np.array(lens) - W, min_len=2, bin=5)
                    assert mismatches(_stats_triple(stats, cover), want) == 0, (L, W, plan, lens)
                    assert torch.equal(ll, ll2), (L, W, plan, lens)


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_sample_grouping_slabs_repeats_masks_classes_and_indices(dbl):
    from phlash_amd.kernel import get_kernel

    K, L, W = 16, 2000, 100
    rows = _rows(3, L, seed=5, het=0.05, run=300)
    pop = _population(K, 3, seed=7)
    pp = _bcast(pop)
    inds = np.arange(3)
    member = younger_states(K)
    kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
    eng = kern._eng
    ll0, g0 = kern(pp, inds, grad=True)
    plan0 = eng.get_plan()
    kw = dict(in_set=member, seed=7, edges=(3, 10, 40), min_len=4, bin=64)
    free = kern.sample_tracts(pp, inds, n_samples=5, **kw)
    ll1, g1 = kern(pp, inds, grad=True)
    assert eng.get_plan() == plan0 and torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert free.counts.shape == (3, 3, 5, 4) and free.hist.shape == (3, 3, 5, 4) and free.cover.shape == (3, 3, (L - W + 63) // 64)
    eng.set_plan(0, 4, 8, 4, 0)  # (a slab is a launch shape of its own: fix the plan so that every run below uses the same one)
    fixed = eng.get_plan()
    five = kern.sample_tracts(pp, inds, n_samples=5, **kw)
    stored = kern.sample_paths(pp, inds, n_samples=5, seed=7)
    assert torch.equal(five.ll, stored.ll)
    # sample grouping: row r does not depend on n_samples; cover is the sum of the samples' own
    for n in (1, 2):
        few = kern.sample_tracts(pp, inds, n_samples=n, **kw)
        assert torch.equal(few.counts, five.counts[:, :, :n]) and torch.equal(few.hist, five.hist[:, :, :n]), n
        single = [_pt(stored.paths[:, :, r : r + 1], member, edges=(3, 10, 40), min_len=4, bin=64) for r in range(n)]
        assert torch.equal(few.cover, sum(s.cover for s in single)), n
    single = [_pt(stored.paths[:, :, r : r + 1], member, edges=(3, 10, 40), min_len=4, bin=64) for r in range(5)]
    assert torch.equal(five.cover, sum(s.cover for s in single))
    assert torch.equal(five.counts, torch.cat([s.counts for s in single], 2)) and torch.equal(five.hist, torch.cat([s.hist for s in single], 2))
    assert int(five.hist[..., 1:].sum()) > 0 and int(five.cover.sum()) > 0
    # slabs (by particles, by chunks; the difference rows of cover are part of the slab arithmetic) and repeats
    per_seq = ((L + 7) // 8) * K * (8 if dbl else 4) + 4 * five.cover.shape[-1]
    for nseq in (4, 2):
        eng.set_workspace_limit(per_seq * nseq + 1)
        for _ in range(2):
            d = kern.sample_tracts(pp, inds, n_samples=5, **kw)
            assert mismatches(_triple(d), _triple(five)) == 0 and torch.equal(d.ll, five.ll), nseq
    eng.set_workspace_limit(1 << 40)
    again = kern.sample_tracts(pp, inds, n_samples=5, **kw)
    assert mismatches(_triple(again), _triple(five)) == 0 and eng.get_plan() == fixed
    # masks.  Empty: only the changes of state are left
    changes = (stored.paths[..., 1:] != stored.paths[..., :-1]).sum(-1).to(torch.int32)
    e = kern.sample_tracts(pp, inds, in_set=np.zeros(K, bool), n_samples=5, seed=7, edges=(3,), bin=64)
    assert int(e.counts[..., :3].abs().sum()) == 0 and int(e.hist.abs().sum()) == 0 and int(e.cover.abs().sum()) == 0
    assert torch.equal(e.counts[..., 3], changes) and torch.equal(five.counts[..., 3], changes)
    # full: one tract of len - W sites, cover = n_samples x the bin's own sites
    lens = np.array([L, 1234, W + 1])
    f = kern.sample_tracts(pp, inds, in_set=np.ones(K, bool), n_samples=5, seed=7, edges=(1234 - W,), lens=lens, bin=64)
    own = torch.as_tensor(lens - W, device=f.counts.device)
    assert torch.equal(f.counts[..., 0].long(), own[None, :, None].expand(3, 3, 5)) and torch.equal(f.counts[..., 2], f.counts[..., 0])
    assert int((f.counts[..., 1] != 1).sum()) == 0
    assert f.hist[:, 0, :, 1].eq(1).all() and f.hist[:, 1, :, 1].eq(1).all() and f.hist[:, 2, :, 0].eq(1).all()  # (1234 - W: on the edge)
    sites = (own[:, None] - 64 * torch.arange(f.cover.shape[-1], device=own.device)[None]).clamp(0, 64)
    assert torch.equal(f.cover.long(), (5 * sites)[None].expand(3, -1, -1))
    # one mask per particle, against one call per particle's mask
    per = np.stack([member, ~member, np.arange(K) % 3 == 0])
    m = kern.sample_tracts(pp, inds, in_set=per, n_samples=5, seed=7, edges=(3, 10, 40), min_len=4, bin=64, lens=lens)
    for b in range(3):
        alone = kern.sample_tracts(pp, inds, in_set=per[b], n_samples=5, seed=7, edges=(3, 10, 40), min_len=4, bin=64, lens=lens)
        assert mismatches((m.counts[b], m.hist[b], m.cover[b]), (alone.counts[b], alone.hist[b], alone.cover[b])) == 0, b
    want = _pt(stored.paths, per, edges=(3, 10, 40), lens=lens - W, min_len=4, bin=64)
    assert mismatches(_triple(m), want) == 0
    # edge classes: none and fifteen; the histogram sums to the tracts, its lengths to the sites inside
    z = kern.sample_tracts(pp, inds, n_samples=5, in_set=member, seed=7)
    assert z.hist.shape == (3, 3, 5, 1) and torch.equal(z.hist[..., 0], z.counts[..., 1]) and z.cover is None
    assert torch.equal(z.counts, five.counts)
    x = kern.sample_tracts(pp, inds, n_samples=5, in_set=member, seed=7, edges=EDGES15)
    w15 = _pt(stored.paths, member, edges=EDGES15)
    assert x.hist.shape == (3, 3, 5, 16) and torch.equal(x.hist.sum(-1), x.counts[..., 1]) and mismatches((x.counts, x.hist), (w15.counts, w15.hist)) == 0
    # (classes 0 .. 14 hold the lengths 0 .. 14 exactly: with the rest in class 15 they account for column 0)
    short = (x.hist[..., :15].long() * torch.arange(15, device=x.hist.device)).sum(-1)
    assert bool((short <= x.counts[..., 0]).all()) and bool(((x.hist[..., 15] == 0).int() <= (short == x.counts[..., 0]).int()).all())
    # permuted and repeated inds: the draws follow the position in the call, the data and lens follow the data row
    px = kern.sample_tracts(pp, np.array([2, 0, 2]), lens=lens, n_samples=3, **kw)
    sx = kern.sample_paths(pp, np.array([2, 0, 2]), n_samples=3, seed=7)
    wx = _pt(sx.paths, member, edges=(3, 10, 40), lens=lens[[2, 0, 2]] - W, min_len=4, bin=64)
    assert mismatches(_triple(px), wx) == 0 and torch.equal(px.ll, sx.ll)
    assert int(px.counts[:, 0, :, 0].max()) <= 1 and int(px.counts[:, 1, :, 0].max()) > 1  # (row 2: one own reported site)


@pytest.mark.gpu
def test_phk_sample_tracts_argument_checks_on_a_live_handle():
    """every check of the header comment, each refused with PHK_EINVAL before anything is enqueued: the outputs keep their fill"""
    import ctypes

    from phlash_amd import _lib
    from phlash_amd.engine import HipEngine

    K, L, S = 8, 40, 2
    eng = HipEngine(K, _rows(S, L, seed=9, het=0.1), double_precision=True)
    c = eng._sweep_call(_params(_population(K, 2, seed=3)), torch.arange(S, device="cuda"))
    masks = _mask_words(younger_states(K))
    ll = torch.full((2, S), 7.0, dtype=torch.float64, device="cuda")
    stats = torch.full((2, S, 1, 6), 7, dtype=torch.int32, device="cuda")
    cover = torch.full((2, S, L), 7, dtype=torch.int32, device="cuda")
    lib = _lib.load()

    def call(W=0, n=1, mp=masks.data_ptr(), edges=(3,), n_edges=None, bin=1, min_len=1, llp=ll.data_ptr(), sp=stats.data_ptr(),
             cp=cover.data_ptr(), head=c.head, inds=c.grid[0]):
        arr = (ctypes.c_int64 * 16)(*edges)
        return lib.phk_sample_tracts(*head, inds, c.B, c.S, W, n, 0, mp, 0, None, arr, len(edges) if n_edges is None else n_edges, bin, min_len,
                                     llp, sp, cp, c.stream)

    bad = [dict(head=(c.head[0], None) + c.head[2:]), dict(inds=None), dict(llp=None), dict(sp=None), dict(mp=None),
           dict(W=-1), dict(W=L), dict(n=0), dict(n=65536), dict(n_edges=-1), dict(edges=tuple(range(1, 17))), dict(edges=(3, 3)),
           dict(edges=(5, 4)), dict(edges=(0, 4)), dict(bin=0), dict(min_len=0)]  # (n_samples x min(bin, L - W) >= 2^31 needs a row of 32,769 sites: not built here)
    for kw in bad:
        assert call(**kw) == _lib.PHK_EINVAL, kw
        assert lib.phk_last_error(), kw
    assert call(W=L) == _lib.PHK_EINVAL and lib.phk_last_error() == f"W={L} outside [0, L={L})".encode()  # phk_sample_paths' words
    torch.cuda.synchronize()
    assert bool((ll == 7).all()) and bool((stats == 7).all()) and bool((cover == 7).all())
    # bin and min_len are not looked at without cover; the call itself is fine
    assert call(bin=0, min_len=0, cp=None) == _lib.PHK_OK and call() == _lib.PHK_OK
    torch.cuda.synchronize()
    assert not eng.underflow_risk() and bool((stats[..., 1] == stats[..., 4:].sum(-1)).all()) and int(cover.sum()) == int(stats[..., 0].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [True, False])
def test_statistical_anchors_against_the_exact_sweeps(dbl):
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    pp, row, _, _ = stat_inputs()
    member = younger_states(8)
    kern = get_kernel(8, row[None], double_precision=dbl)
    q = PSMCParams(*(torch.as_tensor(x) for x in pp))
    out = kern.sample_tracts(q, np.int64(0), in_set=member, n_samples=STAT_N, seed=STAT_SEED, min_len=1, bin=STAT_BIN)
    assert out.counts.shape == (STAT_N, 4) and out.cover.shape == (len(row) // STAT_BIN,) and out.ll.shape == ()
    marg = kern.posterior(q, np.int64(0), bin=1).marginals.double().cpu().numpy()[:, member].sum(1)  # [96]
    chg = kern.transitions(q, np.int64(0), bin=1, arrivals=False).changes.double().cpu().numpy()  # [96, 2]
    c = out.counts.cpu().numpy()
    inside = se_score(c[:, 0], marg.sum())
    changes = se_score(c[:, 3], chg[1:].sum())  # (site 0's move comes from z_0, which is no reported site)
    cov = cover_scores(out.cover.cpu().numpy(), STAT_N, marg.reshape(-1, STAT_BIN).sum(1), stat_reference(not dbl)["bin_sd"])
    print(f"STAT tracts {'f64' if dbl else 'f32'}: inside {inside:.2f}, changes {changes:.2f}, worst bin of cover {cov.max():.2f} "
          f"standard errors (the bar is {SE_BAR:g})")
    assert inside < SE_BAR and changes < SE_BAR and cov.max() < SE_BAR
    if dbl:  # the float64 kernel makes the oracle's draws
        assert mismatches(_triple(out), stat_reference(False)["res"]) == 0


@pytest.mark.gpu
def test_tract_lengths_on_two_ragged_contigs_and_two_models():
    import phlash_amd
    from phlash_amd.size_history import DemographicModel

    ws, K, n = 100, 8, 16
    dms = [DemographicModel.default(f"{K}*1", th / ws, 0.04 / ws) for th in (0.05, 0.08)]
    short, full = _rows(2, 60, seed=31, het=0.1), _rows(1, 96, seed=32, het=0.1)
    t_max = float(torch.as_tensor(dms[0].eta.t).reshape(-1)[K - 2])  # (the states 0 .. K - 3 are inside)
    r = phlash_amd.tract_lengths(dms, [short, full], t_max, n_samples=n, seed=5, edges=(2, 5), min_len=3, bin=10, window_size=ws)
    assert isinstance(r, phlash_amd.TractLengths)
    assert r.spectrum.mean.shape == r.spectrum.lo.shape == r.spectrum.hi.shape == (3, 3)
    for s in (r.n_tracts, r.longest, r.inside):
        assert s.mean.shape == s.lo.shape == s.hi.shape == (3,) and bool((s.lo <= s.mean).all()) and bool((s.mean <= s.hi).all())
    assert r.counts.shape == (2, 3, n, 4) and r.hist.shape == (2, 3, n, 3)
    assert [tuple(x.shape) for x in r.in_long] == [(2, 6), (1, 10)]
    assert all(bool(((x >= 0) & (x <= 1)).all()) for x in r.in_long)
    assert torch.allclose(r.spectrum.mean.sum(-1), r.n_tracts.mean, rtol=1e-12, atol=0)
    assert bool((r.longest.hi[:2] <= 60).all()) and bool((r.inside.hi[:2] <= 60).all())  # the padding of the short rows counts for nothing
    assert float(r.inside.mean.max()) > 0 and float(r.n_tracts.mean.max()) > 0
    # a matrix; the full set at min_len = 1: every own window lies in the one tract
    f = phlash_amd.tract_lengths(dms, [short, full], 0.0, n_samples=n, seed=5, edges=(2, 5), min_len=1, bin=10, window_size=ws,
                                 in_set=np.ones(K, bool))
    assert all(bool((x == 1).all()) for x in f.in_long)
    assert f.n_tracts.mean.tolist() == [1.0, 1.0, 1.0] and f.longest.mean.tolist() == [60.0, 60.0, 96.0]
    g = phlash_amd.tract_lengths(dms[0], full, t_max, n_samples=n, seed=5, bin=10, min_len=3, window_size=ws)
    assert g.in_long.shape == (1, 10) and g.spectrum.mean.shape == (1, 4) and g.counts.shape == (1, 1, n, 4)
