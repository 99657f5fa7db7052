"""Posterior path sampling (phk_sample_paths / HipEngine.sample_paths / PSMCKernel.sample_paths / phlash_amd.sample_tmrca).

CPU: the Philox known answers and the two uniform formulas, the float64 oracle (tests/sampling_oracle.py) against path
enumeration, the margin condition that makes exact path equality meaningful on the GPU tests' inputs, the statistical bars on
the oracle's own draws, the comparators against injected faults, the ABI's argument check without a device, the re-export.
GPU: float64 paths equal to the oracle's at every site, sample and sequence; float32 paths equal up to a draw the oracle itself
decides by less than float32 keeps; block and unit edges; identities that tie the call to the shipped ones; the statistical
bars on the kernels' draws; sample_tmrca.
"""

from __future__ import annotations

import functools
import warnings

import numpy as np
import pytest
import torch

import posterior_oracle as po
import sampling_oracle as so
from decode_fuzz import F32_GAMMA_BAR
from oracle import psmc_numpy as pn
from test_viterbi import GRID_K, _bcast, _per_chunk, _population, _pp_np, _random_pp, _rows, grid_block, grid_inputs

# Exact path equality is only meaningful where no draw of the oracle falls closer than this to a boundary of its CDF (relative to
# the total): the float64 kernels' weights differ from the oracle's by a few roundings each (1e-15).  Asserted on the oracle.
MIN_MARGIN = 1e-7
GRID_SEED = 1234
GRID_SAMPLES = 4
GRID_W = (0, 37)
# the statistical input: one row of 96 windows, K = 8
STAT_N, STAT_SEED, STAT_PAIR = 4096, 77, 39


# ------------------------------------------------------------------------------------------------- shared references
@functools.lru_cache(maxsize=None)
def grid_reference(K, bits24=False):
    """{(W, layout): (paths [B][S] of uint8 [n, L - W], margins likewise, ll [B, S])} on test_viterbi.grid_inputs(K), rows at
    full length, computed once and shared (read only)"""
    pp, pc, sets = grid_inputs(K)
    out = {}
    for (rows, _, _), W in zip(sets, GRID_W):
        S = len(rows)
        for layout in ("bcast", "chunk"):
            paths, margins, ll = [], [], np.empty((2, S))
            for b in range(2):
                ps, ms = [], []
                for s in range(S):
                    q = grid_block(pp, pc, layout, b, s)
                    alpha, ll[b, s] = so.forward(q, rows[s], W=W)
                    p, m = so.sample(q, rows[s], W, b * S + s, GRID_SAMPLES, GRID_SEED, bits24=bits24, alpha=alpha)
                    ps.append(p)
                    ms.append(m)
                paths.append(ps)
                margins.append(ms)
            out[W, layout] = (paths, margins, ll)
    return out


EDGE_K, EDGE_B, EDGE_S, EDGE_SAMPLES, EDGE_SEED = 16, 2, 2, 3, 4321
EDGE_L = (1, 15, 16, 17, 33, 130)


def edge_rows(L):
    return _rows(EDGE_S, L, seed=100 + L, het=0.1, run=L // 3 if L >= 15 else None)


@functools.lru_cache(maxsize=None)
def edge_reference(L, W, bits24=False):
    """(paths [B][S], margins [B][S], ll [B, S]) of the block-edge shapes: K = 16, a run of missing windows per row"""
    pop = _population(EDGE_K, EDGE_B, seed=11)
    rows = edge_rows(L)
    paths, margins, ll = [], [], np.empty((EDGE_B, EDGE_S))
    for b in range(EDGE_B):
        q = _pp_np(pop, b)
        ps, ms = [], []
        for s in range(EDGE_S):
            alpha, ll[b, s] = so.forward(q, rows[s], W=W)
            p, m = so.sample(q, rows[s], W, b * EDGE_S + s, EDGE_SAMPLES, EDGE_SEED, bits24=bits24, alpha=alpha)
            ps.append(p)
            ms.append(m)
        paths.append(ps)
        margins.append(ms)
    return paths, margins, ll


def edge_cases():
    return [(L, W) for L in EDGE_L for W in sorted({0, L - 1})]


@functools.lru_cache(maxsize=None)
def stat_inputs():
    pp = _random_pp(8, np.random.default_rng(5))
    row = _rows(1, 96, seed=3, het=0.1)[0]
    gamma, _ = po.forward_backward(pp, row, 0)
    xi = so.pair_posterior(pp, row, STAT_PAIR)
    return pp, row, gamma, xi


def _params(pop):
    return torch.stack([torch.as_tensor(a) for a in pop], -2)[:, None].cuda()  # [B, 1, 7, K]


# ------------------------------------------------------------------------------------------------- CPU
def test_philox_known_answers_and_the_uniform_formulas():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = tuple(int(x) for x in so.philox4x32_10(ctr, key))
        assert got == want, ([hex(x) for x in got], [hex(x) for x in want])
    # vectorised over counters: the same words
    x = so.philox4x32_10((np.array([0, 0x243F6A88]), np.array([0, 0x85A308D3]), np.array([0, 0x13198A2E]), np.array([0, 0x03707344])), (0, 0))
    assert int(x[0][0]) == 0x6627E8D5
    # x0 = 0x80000100, x1 = 0x00001800: U53 = 2^-1 + 2^-24 + 3 * 2^-53 (x1 >> 11 = 3), U24 = 2^-1 + 2^-24
    assert float(so.u53(0x80000100, 0x00001800)) == 0.5 + 2.0 ** -24 + 3 * 2.0 ** -53
    assert float(so.u24(0x80000100)) == 0.5 + 2.0 ** -24
    assert float(so.u24(0x800001FF)) == 0.5 + 2.0 ** -24  # the low 8 bits are dropped
    assert float(so.u53(0xFFFFFFFF, 0xFFFFFFFF)) == 1.0 - 2.0 ** -53 and float(so.u24(0xFFFFFFFF)) == 1.0 - 2.0 ** -24
    # uniforms(): counter (t, r, q lo, q hi), key (seed lo, seed hi)
    q, seed = (5 << 32) | 7, (9 << 32) | 11
    U = so.uniforms(seed, q, [0, 3], [2, 6])
    w = so.philox4x32_10((6, 3, 7, 5), (11, 9))
    assert U.shape == (2, 2) and U[1, 1] == float(so.u53(w[0], w[1]))
    assert so.uniforms(seed, q, [0, 3], [2, 6], bits24=True)[1, 1] == float(so.u24(w[0]))


@pytest.mark.parametrize("K,L,W", [(2, 5, 0), (3, 5, 2), (3, 4, 0), (2, 4, 2)])
def test_oracle_against_path_enumeration(K, L, W):
    rng = np.random.default_rng(K * 10 + L + W)
    pp = _random_pp(K, rng)
    data = rng.integers(0, 2, size=L)
    data[0] = 1
    data[L // 2] = -1  # a missing site
    N = 20_000
    probs = so.path_probabilities(pp, data, W)
    assert abs(sum(probs.values()) - 1) < 1e-12 and len(probs) == K ** (L - W)
    paths, margins = so.sample(pp, data, W, q=3, n_samples=N, seed=99)
    assert paths.shape == (N, L - W) and margins.shape == paths.shape and (margins >= 0).all()
    keys, counts = np.unique(paths, axis=0, return_counts=True)
    freq = {tuple(int(z) for z in k): c / N for k, c in zip(keys, counts)}
    assert set(freq) <= set(probs)
    for path, p in probs.items():
        f = freq.get(path, 0.0)
        assert abs(f - p) <= 6 * np.sqrt(p * (1 - p) / N), (path, f, p)
    # sample r is a function of (seed, q, r, site): not of n_samples; other q or seed: other draws
    few, _ = so.sample(pp, data, W, q=3, n_samples=5, seed=99)
    assert np.array_equal(few, paths[:5])
    U = so.uniforms(99, 3, np.arange(5), np.arange(L))
    assert np.array_equal(U, so.uniforms(99, 3, np.arange(N), np.arange(L))[:, :5])
    assert (U != so.uniforms(99, 4, np.arange(5), np.arange(L))).all() and (U != so.uniforms(98, 3, np.arange(5), np.arange(L))).all()


@pytest.mark.parametrize("K", GRID_K)
def test_margin_condition_of_the_gpu_grid(K):
    ref = grid_reference(K)
    worst = min(float(m.min()) for paths, margins, _ in ref.values() for ms in margins for m in ms)
    print(f"MARGIN sampling K={K}: smallest margin of the grid {worst:.2e}")
    for (W, layout), (paths, margins, _) in ref.items():
        low = min(float(m.min()) for ms in margins for m in ms)
        assert low >= MIN_MARGIN, f"K={K} W={W} {layout}: margin {low:.2e} -- pick another GRID_SEED"
        assert all(p.shape == (GRID_SAMPLES, 700 - W) and int(p.max()) < K for ps in paths for p in ps)


@pytest.mark.parametrize("K", GRID_K)
def test_structured_draw_gives_the_oracle_paths_on_the_gpu_inputs(K):
    """the folded O(K) form of the weights and the lane-wise prefix sums the kernels use, in float64 loops, against the dense
    oracle: one (particle, chunk) pair per data set and layout"""
    pp, pc, sets = grid_inputs(K)
    ref = grid_reference(K)
    for (rows, _, _), W in zip(sets, GRID_W):
        for layout, b, s in (("bcast", 1, 2), ("chunk", 0, 1)):
            q = grid_block(pp, pc, layout, b, s)
            got = so.structured_sample(q, rows[s], W, b * len(rows) + s, 2, GRID_SEED)
            assert so.count_unequal(ref[W, layout][0][b][s][:2], got) == 0, (K, W, layout)


def test_margin_condition_of_the_edge_shapes():
    worst = np.inf
    for L, W in edge_cases():
        _, margins, _ = edge_reference(L, W)
        low = min(float(m.min()) for ms in margins for m in ms)
        assert low >= MIN_MARGIN, f"L={L} W={W}: margin {low:.2e} -- pick another EDGE_SEED"
        worst = min(worst, low)
    print(f"MARGIN sampling, edge shapes: smallest margin {worst:.2e}")


def test_statistical_bars_on_the_oracle():
    pp, row, gamma, xi = stat_inputs()
    paths, _ = so.sample(pp, row, 0, q=0, n_samples=STAT_N, seed=STAT_SEED)
    site, pair = so.site_score(paths, gamma), so.pair_score(paths, STAT_PAIR, xi)
    print(f"STAT sampling oracle: site score {site:.3f}, pair score {pair:.3f} (a pass is < 1)")
    assert site < 1 and pair < 1
    p24, _ = so.sample(pp, row, 0, q=0, n_samples=STAT_N, seed=STAT_SEED, bits24=True)
    assert so.site_score(p24, gamma) < 1 and so.pair_score(p24, STAT_PAIR, xi) < 1
    assert abs(xi.sum(1) - gamma[STAT_PAIR]).max() < 1e-12 and abs(xi.sum(0) - gamma[STAT_PAIR + 1]).max() < 1e-12


def test_comparators_fail_on_injected_faults():
    pp, row, gamma, xi = stat_inputs()
    paths, margins = so.sample(pp, row, 0, q=0, n_samples=STAT_N, seed=STAT_SEED)
    assert so.count_unequal(paths, paths) == 0
    # samples swapped: every site-wise statistic is unchanged, the parity comparators are not
    swapped = paths.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert so.site_score(swapped, gamma) == so.site_score(paths, gamma)
    assert so.count_unequal(paths, swapped) > 0
    p24, m24 = so.sample(pp, row, 0, q=0, n_samples=8, seed=STAT_SEED, bits24=True)
    assert so.f32_divergences(pp, row, 0, p24, m24, p24, F32_GAMMA_BAR) == (0, [])
    sw24 = p24.copy()
    sw24[[0, 1]] = sw24[[1, 0]]
    n, bad = so.f32_divergences(pp, row, 0, p24, m24, sw24, F32_GAMMA_BAR)
    assert n == 2 and len(bad) == 2
    # sites shifted by one
    shifted = np.roll(paths, 1, axis=1)
    assert so.count_unequal(paths, shifted) > 0
    n, bad = so.f32_divergences(pp, row, 0, p24, m24, np.roll(p24, 1, axis=1), F32_GAMMA_BAR)
    assert n > 0 and len(bad) > 0
    # draws taken independently from gamma: right at every site, wrong jointly
    rng = np.random.default_rng(0)
    indep = (rng.random((STAT_N, len(row)))[:, :, None] > np.cumsum(gamma, 1)[None, :, : gamma.shape[1] - 1]).sum(2)
    assert so.site_score(indep, gamma) < 1
    assert so.pair_score(indep, STAT_PAIR, xi) >= 1
    # a chain under another model misses the site bar
    other = pn.from_dm(pn.DM(t=np.concatenate([[0.0], np.geomspace(1e-3, 8.0, 7)]), c=np.ones(8), theta=0.5, rho=0.02))
    wrong, _ = so.sample(other, row, 0, q=0, n_samples=STAT_N, seed=STAT_SEED)
    assert so.site_score(wrong, gamma) >= 1


def test_phk_sample_paths_rejects_bad_arguments_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_sample_paths" in _lib.SIGNATURES
    rc = lib.phk_sample_paths(None, None, 0, 0, None, None, 1, 1, 0, 1, 0, None, None, 0, None)
    assert rc == _lib.PHK_EINVAL
    assert b"NULL" in lib.phk_last_error()


def test_sample_tmrca_is_lazy_and_has_no_cpu_fallback(monkeypatch):
    import phlash_amd

    f = phlash_amd.sample_tmrca
    from phlash_amd.decode import sample_tmrca

    assert f is sample_tmrca
    from phlash_amd.kernel import PathSample, PSMCKernel

    assert hasattr(PSMCKernel, "sample_paths") and PathSample._fields == ("ll", "paths")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dm = phlash_amd.DemographicModel.default("4*1", 1e-4, 1e-4)
    data = np.zeros((1, 50), dtype=np.int8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        sample_tmrca(dm, data)


# ------------------------------------------------------------------------------------------------- GPU
def _grid_calls(K, dbl):
    """every call of the grid: yields (W, layout, rows, paths_gpu [B, S, n, L - W], ll_gpu [B, S])"""
    from phlash_amd.kernel import get_kernel

    pp, pc, sets = grid_inputs(K)
    for (rows, _, _), W in zip(sets, GRID_W):
        S, L = rows.shape
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        for layout in ("bcast", "chunk"):
            q = _bcast(pp) if layout == "bcast" else _per_chunk(pc, S)
            with warnings.catch_warnings():
                warnings.simplefilter("error")  # ordinary parameters: no underflow flag, no re-evaluation
                out = kern.sample_paths(q, np.arange(S), n_samples=GRID_SAMPLES, seed=GRID_SEED)
            assert out.paths.shape == (2, S, GRID_SAMPLES, L - W) and out.paths.dtype == torch.uint8 and out.ll.shape == (2, S)
            yield W, layout, rows, out.paths.cpu().numpy(), out.ll.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("K", GRID_K)
def test_f64_paths_equal_the_oracle_at_every_site(K):
    ref = grid_reference(K)
    worst = 0.0
    for W, layout, rows, paths, ll in _grid_calls(K, True):
        rp, rm, rll = ref[W, layout]
        assert min(float(m.min()) for ms in rm for m in ms) >= MIN_MARGIN
        for b in range(2):
            for s in range(len(rows)):
                diff = so.count_unequal(rp[b][s], paths[b, s])
                assert diff == 0, f"K={K} W={W} b={b} s={s} {layout}: {diff} of {paths[b, s].size} entries differ from the oracle's paths"
        worst = max(worst, float(np.abs(ll / rll - 1).max()))
    print(f"PARITY sampling K={K} f64: paths equal at every site, sample and sequence; max rel ll error {worst:.3e}")
    assert worst < 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("K", GRID_K)
def test_f32_paths_equal_the_oracle_up_to_a_draw_float32_cannot_decide(K):
    pp, pc, _ = grid_inputs(K)
    ref = grid_reference(K, True)
    diverged, total, worst_ll = 0, 0, 0.0
    for W, layout, rows, paths, ll in _grid_calls(K, False):
        rp, rm, rll = ref[W, layout]
        assert int(paths.max()) < K
        for b in range(2):
            for s in range(len(rows)):
                n, bad = so.f32_divergences(grid_block(pp, pc, layout, b, s), rows[s], W, rp[b][s], rm[b][s], paths[b, s], F32_GAMMA_BAR)
                assert not bad, f"K={K} W={W} b={b} s={s} {layout}: (sample, site, oracle margin, bar) {bad}"
                diverged += n
                total += GRID_SAMPLES
        worst_ll = max(worst_ll, float(np.abs(ll / rll - 1).max()))
    print(f"PARITY sampling K={K} f32: {diverged} of {total} paths diverged from the oracle's (each at a draw within the bar); "
          f"max rel ll error {worst_ll:.3e}")
    assert worst_ll < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [True, False])
def test_block_and_unit_edges(dbl):
    from phlash_amd.engine import HipEngine

    pop = _population(EDGE_K, EDGE_B, seed=11)
    P = _params(pop)
    inds = torch.arange(EDGE_S, device="cuda")
    plans = [(0, 4, 8, 4, 0), (0, 4, 16, 4, 0)] + ([] if dbl else [(0, 4, 8, 16, 0)])  # the last: one state per lane forward kernel
    diverged = 0
    for L in EDGE_L:
        rows = edge_rows(L)
        eng = HipEngine(EDGE_K, rows, double_precision=dbl)
        for W in sorted({0, L - 1}):
            rp, rm, rll = edge_reference(L, W, bits24=not dbl)
            for plan in plans:
                eng.set_plan(*plan)
                ll, paths = eng.sample_paths(P, inds, warmup=W, n_samples=EDGE_SAMPLES, seed=EDGE_SEED)
                assert not eng.underflow_risk()
                assert paths.shape == (EDGE_B, EDGE_S, EDGE_SAMPLES, L - W)
                paths, ll = paths.cpu().numpy(), ll.cpu().numpy()
                for b in range(EDGE_B):
                    for s in range(EDGE_S):
                        if dbl:
                            assert so.count_unequal(rp[b][s], paths[b, s]) == 0, (L, W, plan, b, s)
                        else:
                            n, bad = so.f32_divergences(_pp_np(pop, b), rows[s], W, rp[b][s], rm[b][s], paths[b, s], F32_GAMMA_BAR)
                            assert not bad, (L, W, plan, b, s, bad)
                            diverged += n
                assert np.abs(ll - rll).max() <= (1e-13 if dbl else 1e-5) * max(1.0, np.abs(rll).max()), (L, W, plan)
    if not dbl:
        print(f"PARITY sampling edges f32: {diverged} paths diverged from the oracle's (each at a draw within the bar)")


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_identities(dbl):
    from phlash_amd.kernel import get_kernel

    K, L, W = 16, 2000, 100
    rows = _rows(3, L, seed=5, het=0.05, run=300)
    pp = _bcast(_population(K, 3, seed=7))
    inds = np.arange(3)
    kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
    eng = kern._eng
    # a gradient call before and after: identical bits, plan untouched
    ll0, g0 = kern(pp, inds, grad=True)
    plan0 = eng.get_plan()
    a = kern.sample_paths(pp, inds, n_samples=3, seed=7)
    ll1, g1 = kern(pp, inds, grad=True)
    assert torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert eng.get_plan() == plan0
    assert a.paths.shape == (3, 3, 3, L - W) and int(a.paths.max()) < K
    # ll is the forward leg's by-product: phk_posterior's, to the bit, under the same (forced) plan
    for plan in ((0, 4, 8, 4, 0), (0, 4, 16, 4, 0), (1, 4, 8, 4, 4)):
        eng.set_plan(*plan)
        s = kern.sample_paths(pp, inds, n_samples=2, seed=7)
        p = kern.posterior(pp, inds, bin=50)
        assert torch.equal(s.ll, p.ll), plan
    eng.set_plan(0, 4, 8, 4, 0)  # (a slab is a launch shape of its own: fix the plan so that every run below uses the same one)
    a = kern.sample_paths(pp, inds, n_samples=3, seed=7)
    # same seed, same bytes; another seed, other draws; sample r does not depend on n_samples
    b = kern.sample_paths(pp, inds, n_samples=3, seed=7)
    assert torch.equal(a.paths, b.paths) and torch.equal(a.ll, b.ll)
    c = kern.sample_paths(pp, inds, n_samples=3, seed=8)
    assert not torch.equal(a.paths, c.paths) and torch.equal(a.ll, c.ll)
    five = kern.sample_paths(pp, inds, n_samples=5, seed=7)
    assert torch.equal(five.paths[:, :, :3], a.paths)
    one = kern.sample_paths(pp, inds, n_samples=1, seed=7)
    assert torch.equal(one.paths[:, :, 0], a.paths[:, :, 0])
    assert not torch.equal(five.paths[:, :, 3], five.paths[:, :, 4])
    # slabs: by particles (4 sequences per slab: one particle), by chunks (2 per slab)
    per_seq = ((L + 7) // 8) * K * (8 if dbl else 4)
    for nseq in (4, 2):
        eng.set_workspace_limit(per_seq * nseq + 1)
        d = kern.sample_paths(pp, inds, n_samples=3, seed=7)
        assert torch.equal(a.paths, d.paths) and torch.equal(a.ll, d.ll), nseq
    eng.set_workspace_limit(1 << 40)
    # permuted and repeated inds: the draws follow q = b * S + s, the position in the call, and the data follow inds
    x = kern.sample_paths(pp, np.array([2, 0, 2]), n_samples=3, seed=7)
    y = kern.sample_paths(pp, np.array([1, 0, 1]), n_samples=3, seed=7)
    assert torch.equal(x.paths[:, 1], y.paths[:, 1]) and torch.equal(x.ll[:, 1], y.ll[:, 1])
    assert not torch.equal(x.paths[:, 0], x.paths[:, 2]) and torch.equal(x.ll[:, 0], x.ll[:, 2])
    assert torch.equal(x.paths[:, 2], a.paths[:, 2])  # (row 2 at position 2 in both)
    assert not torch.equal(x.paths[:, 1], a.paths[:, 0])  # (row 0 at position 1 / at position 0)


@pytest.mark.gpu
def test_f64_paths_follow_q_by_call_position():
    """permuted and repeated ``inds`` against the oracle: sequence (b, s) of the call reads data row inds[s] and draws with
    q = b * S + s"""
    from phlash_amd.kernel import get_kernel

    K, L, W = 8, 130, 5
    rows = _rows(3, L, seed=21, het=0.1)
    pop = _population(K, 2, seed=8)
    inds = np.array([2, 0, 2, 1])
    kern = get_kernel(K, rows, double_precision=True, overlap=W)
    out = kern.sample_paths(_bcast(pop), inds, n_samples=3, seed=555)
    paths = out.paths.cpu().numpy()
    for b in range(2):
        for s, row in enumerate(inds):
            p, m = so.sample(_pp_np(pop, b), rows[row], W, b * len(inds) + s, 3, 555)
            assert float(m.min()) >= MIN_MARGIN, (b, s, float(m.min()))
            assert so.count_unequal(p, paths[b, s]) == 0, (b, s)


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [True, False])
def test_statistical_bars_on_the_kernel_draws(dbl):
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    pp, row, gamma, xi = stat_inputs()
    kern = get_kernel(8, row[None], double_precision=dbl)
    out = kern.sample_paths(PSMCParams(*(torch.as_tensor(x) for x in pp)), np.int64(0), n_samples=STAT_N, seed=STAT_SEED)
    assert out.paths.shape == (STAT_N, len(row)) and out.ll.shape == ()
    paths = out.paths.cpu().numpy()
    site, pair = so.site_score(paths, gamma), so.pair_score(paths, STAT_PAIR, xi)
    print(f"STAT sampling {'f64' if dbl else 'f32'}: site score {site:.3f}, pair score {pair:.3f} (a pass is < 1)")
    assert site < 1 and pair < 1


@pytest.mark.gpu
def test_sample_tmrca_shapes_cut_and_marginals():
    import phlash_amd
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel

    ws, K, N = 100, 8, 2048
    dms = [DemographicModel.default(f"{K}*1", th / ws, 0.04 / ws) for th in (0.05, 0.08)]
    short, full = _rows(2, 60, seed=31, het=0.1), _rows(1, 96, seed=32, het=0.1)
    # one model, a matrix
    p, t = phlash_amd.sample_tmrca(dms[0], full, n_samples=3, seed=5, window_size=ws)
    assert p.shape == (1, 3, 96) == t.shape and p.dtype == torch.uint8 and t.dtype == torch.float64
    ect = torch.as_tensor(dms[0].eta.ect(), dtype=torch.float64, device=p.device)
    assert torch.equal(t, ect[p.long()])
    # two models, a ragged list of two contigs
    paths, tmrca = phlash_amd.sample_tmrca(dms, [short, full], n_samples=N, seed=5, window_size=ws)
    assert [tuple(x.shape) for x in paths] == [(2, 2, N, 60), (2, 1, N, 96)] == [tuple(x.shape) for x in tmrca]
    for b, dm in enumerate(dms):
        ect = torch.as_tensor(dm.eta.ect(), dtype=torch.float64, device=paths[0].device)
        for c in range(2):
            assert int(paths[c][b].max()) < K
            assert torch.equal(tmrca[c][b], ect[paths[c][b].long()])
    # the same call on the matrix of the long contig alone: q and the data of its row differ, the distribution does not;
    # the own-length part of a padded row has the marginals of the row alone
    worst = 0.0
    for b, dm in enumerate(dms):
        per = DemographicModel(eta=dm.eta, theta=float(dm.theta) * ws, rho=float(dm.rho) * ws)
        q = pn.PP(*(np.asarray(x, float) for x in PSMCParams.from_dm(per)))
        for c, mat in enumerate((short, full)):
            for r in range(mat.shape[0]):
                gamma, _ = po.forward_backward(q, mat[r], 0)
                worst = max(worst, so.site_score(paths[c][b, r].cpu().numpy(), gamma))
    print(f"STAT sample_tmrca: worst site score over models, contigs and rows {worst:.3f} (a pass is < 1)")
    assert worst < 1
