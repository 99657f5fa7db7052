"""Viterbi decoding (phk_viterbi / HipEngine.viterbi / PSMCKernel.viterbi / phlash_amd.viterbi_tmrca, tmrca_segments).

CPU: the float64 log-domain oracle against path enumeration and against its own scorer, a loop-form float64 statement of
the STRUCTURED max-product step the kernels run (prefix / suffix maxima with their indices, folded factors) against the
oracle on the GPU tests' inputs, the ABI's argument check without a device, the lazy re-exports, the segment table.
GPU: float64 paths equal to the oracle's at every site, float32 paths within a bar on the probability they give up, rows of
their own length, identities that tie the call to the shipped ones, extreme parameters, one 3,000,001-window row, recovery
of a simulated path.
"""

from __future__ import annotations

import math
import warnings

import numpy as np
import pytest
import torch

import viterbi_oracle as vo
from decode_fuzz import structured_viterbi, sv32
from oracle import psmc_numpy as pn

# Exact path equality is only meaningful away from ties: every input row of the grid below has at least this distance (log
# units) between the best and the second-best candidate at every site and state.  Asserted on the oracle first.
MIN_MARGIN = 1e-9
# float32 kernels: log probability the float32 path gives up against the optimal one, per site of the row, both scored in
# float64.  The rule of tests/parity_bars.py: 5 x the largest value measured on the MI355X over the grid of
# test_f32_path_is_almost_optimal (every K, both parameter layouts, W = 0 / 37, ragged lens) of
#     logp_oracle - path_logp(pp_float64, data, path_gpu):      2.96e-15 per site (K = 4).
# On that grid every float32 path EQUALS the oracle's (0 of 84,000 sites differ; the smallest margin of the grid is 2e-5 log
# units), so the figure is the float64 rounding of the oracle's running sum, not a loss of the kernel: summed term by term
# (viterbi_oracle.deficit: sites where the paths agree contribute exactly 0) the deficit is exactly 0 for every row.  The
# tests assert the term-by-term figure against this bar everywhere, and the formula above as well where the rows are short.
F32_VITERBI_DEFICIT_BAR = 1.48e-14
# float32 logp against the float64 oracle, relative (the project's float32 ll contract); measured worst on the grid 3.46e-7
# (K = 32), on the 3,000,001-window row 1.01e-7
F32_LOGP_BAR = 1e-5

GRID_K = [4, 8, 12, 16, 32, 64]
GRID_SEEDS = {K: (K, 1, 2) for K in GRID_K}  # (population, rows A, rows B): chosen on the CPU so that MIN_MARGIN holds
# population of the "chunk" layout, one model per (particle, chunk), all different: chosen on the CPU in the same way
GRID_CHUNK_SEEDS = {4: 1004, 8: 1008, 12: 1012, 16: 1016, 32: 1032, 64: 1164}  # (the smallest margin of the grid stays 2e-5)
GRID_L = 700
GRID_LENS = (700, 523, 288)


def _random_pp(K, rng):
    """a valid SMC' model with K states (random size history), as the oracle's PP"""
    t = np.concatenate([[0.0], np.geomspace(1e-3, 8.0, K - 1)])
    c = np.exp(rng.normal(0, 0.5, K))
    dm = pn.DM(t=t, c=c, theta=0.05 * math.exp(rng.normal()), rho=0.02)
    return pn.from_dm(dm)


def _population(K, B, seed):
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population

    tmpl, x = particle_population(K, B, seed=seed, sigma=0.25)
    return PSMCParams.from_dm(tmpl.from_flat(x).to_dm())  # fields [B, K] float64


def _rows(S, L, seed, het=0.03, miss=0.01, run=None):
    rng = np.random.default_rng(seed)
    d = (rng.random((S, L)) < het).astype(np.int8)
    d.flat[rng.integers(0, d.size, int(miss * d.size))] = -1
    if run is not None:  # runs of missing windows (an accessibility mask)
        for s in range(S):
            a = rng.integers(0, L - run)
            d[s, a : a + run] = -1
    d[:, 0] = 1
    return d


def _pp_np(pp, b):
    return pn.PP(*(np.asarray(getattr(pp, f)[b].cpu().numpy() if isinstance(getattr(pp, f), torch.Tensor) else getattr(pp, f)[b],
                              float) for f in pn.PP._fields))


def _bcast(pp):
    from phlash_amd.params import PSMCParams

    return PSMCParams(*(torch.as_tensor(a)[:, None] for a in pp))


def _per_chunk(pc, S):
    """fields [B * S, K], one model per (particle, chunk) -> [B, S, K]"""
    from phlash_amd.params import PSMCParams

    return PSMCParams(*(torch.as_tensor(a).reshape(-1, S, a.shape[-1]).contiguous() for a in pc))


def grid_inputs(K):
    """The inputs of the oracle-parity tests for K states: a population of 2 models ("bcast" layout: one block per particle),
    a population of 2 x 3 models ("chunk" layout: one block per (particle, chunk), all different) and two data sets,
    (rows [3, 700], W, lens or None): isolated missing sites at W = 0, full rows; a run of 120 missing windows per row at
    W = 37, rows of their own lengths."""
    ps, sa, sb = GRID_SEEDS[K]
    pp = _population(K, 2, seed=ps)
    pc = _population(K, 2 * 3, seed=GRID_CHUNK_SEEDS[K])
    return pp, pc, [(_rows(3, GRID_L, seed=sa), 0, None), (_rows(3, GRID_L, seed=sb, run=120), 37, np.array(GRID_LENS))]


def grid_block(pp, pc, layout, b, s):
    """the model of (particle b, chunk s) under a layout, as the oracle's PP"""
    return _pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * 3 + s)


def oracle_grid(pp, rows, W, lens, per_chunk=False):
    """-> paths [B][S] (uint8 [len - W]), logp [B, S], smallest margin.  ``per_chunk``: pp holds one model per (particle,
    chunk), [B * S, K]"""
    B = pp.d.shape[0] // (len(rows) if per_chunk else 1)
    paths, logps, margin = [], np.empty((B, len(rows))), np.inf
    for b in range(B):
        ps = []
        for s, row in enumerate(rows):
            q = _pp_np(pp, b * len(rows) + s if per_chunk else b)
            n = len(row) if lens is None else int(lens[s])
            p, lp, m = vo.viterbi(q, row[:n], W)
            ps.append(p)
            logps[b, s] = lp
            margin = min(margin, m)
        paths.append(ps)
    return paths, logps, margin


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K,L,W", [(2, 6, 0), (3, 6, 2), (4, 5, 0), (4, 5, 3)])
def test_oracle_against_path_enumeration(K, L, W):
    rng = np.random.default_rng(K * 10 + L + W)
    pp = _random_pp(K, rng)
    data = rng.integers(-1, 2, size=L)
    data[0] = 1
    data[L // 2] = -1  # a missing site
    path, logp, margin = vo.viterbi(pp, data, W)
    bpath, blogp = vo.bruteforce(pp, data, W)
    assert margin > 0
    assert path.shape == (L - W,) and np.array_equal(path, bpath)
    assert abs(logp - blogp) < 1e-12 * abs(blogp)
    assert abs(vo.path_logp(pp, data, path, W) - logp) < 1e-12 * abs(logp)


def test_oracle_path_scores_its_own_logp():
    rng = np.random.default_rng(3)
    pp = _random_pp(8, rng)
    data = (rng.random(300) < 0.05).astype(int)
    data[rng.integers(0, 300, 5)] = -1
    for W in (0, 40):
        path, logp, _ = vo.viterbi(pp, data, W)
        assert abs(vo.path_logp(pp, data, path, W) - logp) < 1e-12 * abs(logp)
        # any other path scores lower
        other = path.copy()
        other[100] = (other[100] + 1) % 8
        assert vo.path_logp(pp, data, other, W) < logp
    assert vo.viterbi(pp, data, 0)[1] <= pn.psmc_ll(pp, data)[1]  # max <= sum


@pytest.mark.parametrize("K", GRID_K)
def test_structured_step_gives_the_oracle_path_on_the_gpu_inputs(K):
    pp, pc, sets = grid_inputs(K)
    for rows, W, lens in sets:
        for layout in ("bcast", "chunk"):
            paths, logps, margin = oracle_grid(pp, rows, W, lens) if layout == "bcast" else oracle_grid(pc, rows, W, lens, per_chunk=True)
            assert margin >= MIN_MARGIN, f"K={K} W={W} {layout}: margin {margin:.2e} -- pick other seeds (GRID_SEEDS, GRID_CHUNK_SEEDS)"
            for b in range(2):
                for s, row in enumerate(rows):
                    q = grid_block(pp, pc, layout, b, s)
                    n = len(row) if lens is None else int(lens[s])
                    path, logp = structured_viterbi(q, row[:n])
                    assert np.array_equal(path[W:], paths[b][s]), (K, W, b, s, layout)
                    assert abs(logp - logps[b, s]) < 1e-11 * abs(logps[b, s])
                    if layout == "chunk" and s == b:  # ... and in float32 (what F32_VITERBI_DEFICIT_BAR records of this grid)
                        assert np.array_equal(sv32(q, row[:n])[0][W:], paths[b][s]), (K, W, b, s, layout)


def test_phk_viterbi_rejects_a_null_handle_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_viterbi" in _lib.SIGNATURES
    rc = lib.phk_viterbi(None, None, 0, 0, None, None, 1, 1, 0, None, None, None, 0, None)
    assert rc == _lib.PHK_EINVAL
    assert b"NULL" in lib.phk_last_error()


def test_viterbi_tmrca_is_lazy_and_has_no_cpu_fallback(monkeypatch):
    import phlash_amd

    f = phlash_amd.viterbi_tmrca
    from phlash_amd.decode import tmrca_segments, viterbi_tmrca

    assert f is viterbi_tmrca and phlash_amd.tmrca_segments is tmrca_segments
    from phlash_amd.kernel import PSMCKernel

    assert hasattr(PSMCKernel, "viterbi")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dm = phlash_amd.DemographicModel.default("4*1", 1e-4, 1e-4)
    data = np.zeros((1, 50), dtype=np.int8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        viterbi_tmrca(dm, data)


def test_tmrca_segments_on_a_hand_written_path():
    from phlash_amd.decode import tmrca_segments

    path = torch.tensor([[3, 3, 3, 1, 1, 7, 255, 255], [7, 7, 0, 0, 0, 0, 0, 2]], dtype=torch.uint8)
    row, start, end, state, value = tmrca_segments(path, values=np.arange(8) * 0.5)
    assert row.tolist() == [0, 0, 0, 1, 1, 1]
    assert start.tolist() == [0, 3, 5, 0, 2, 7]
    assert end.tolist() == [3, 5, 6, 2, 7, 8]
    assert state.tolist() == [3, 1, 7, 7, 0, 2]
    assert value.tolist() == [1.5, 0.5, 3.5, 3.5, 0.0, 1.0] and value.dtype == torch.float64
    one = tmrca_segments(path[1])  # a single row, no values; the last run of a row does not merge with the next row's first
    assert [x.tolist() for x in one] == [[0, 0, 0], [0, 2, 7], [2, 7, 8], [7, 0, 2]]
    same = tmrca_segments(torch.tensor([[5, 5], [5, 5]], dtype=torch.uint8))
    assert same[0].tolist() == [0, 1] and same[1].tolist() == [0, 0] and same[2].tolist() == [2, 2]


# ------------------------------------------------------------------------------------------------- GPU
def _expand(segs, N, L):
    row, start, end, state = (x.cpu().numpy() for x in segs[:4])
    out = np.full((N, L), 255, dtype=np.uint8)
    for r, a, b, z in zip(row, start, end, state):
        out[r, a:b] = z
    return out


def _valid_path(pp_np, path):
    """every transition of the path has A > 0"""
    A = pn.dense_from_pp(pp_np)
    z = np.asarray(path).astype(int)
    return bool((A[z[:-1], z[1:]] > 0).all())


def _grid_calls(K, dbl):
    """every call of the grid: yields (model of (b, s), b, s, row[:n], W, path_gpu [n - W], tail of the output row, logp_gpu,
    layout)"""
    from phlash_amd.kernel import get_kernel

    pp, pc, sets = grid_inputs(K)
    B = pp.d.shape[0]
    for rows, W, lens in sets:
        S, L = rows.shape
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        for layout in ("bcast", "chunk"):
            q = _bcast(pp) if layout == "bcast" else _per_chunk(pc, S)  # one block per (particle, chunk), all different
            with warnings.catch_warnings():
                warnings.simplefilter("error")  # ordinary parameters: no underflow flag, no re-evaluation
                out = kern.viterbi(q, np.arange(S), lens=lens)
            assert out.path.shape == (B, S, L - W) and out.path.dtype == torch.uint8 and out.logp.shape == (B, S)
            path, logp = out.path.cpu().numpy(), out.logp.cpu().numpy()
            for b in range(B):
                for s in range(S):
                    n = L if lens is None else int(lens[s])
                    yield grid_block(pp, pc, layout, b, s), b, s, rows[s, :n], W, path[b, s, : n - W], path[b, s, n - W :], logp[b, s], layout


@pytest.mark.gpu
@pytest.mark.parametrize("K", GRID_K)
def test_f64_path_equals_the_oracle_at_every_site(K):
    pp, pc, sets = grid_inputs(K)
    ref = {}
    for rows, W, lens in sets:
        for layout in ("bcast", "chunk"):
            paths, logps, margin = oracle_grid(pp, rows, W, lens) if layout == "bcast" else oracle_grid(pc, rows, W, lens, per_chunk=True)
            assert margin >= MIN_MARGIN, f"K={K} W={W} {layout}: margin {margin:.2e}"
            ref[W, layout] = (paths, logps)
    worst = 0.0
    for _, b, s, row, W, path, tail, logp, layout in _grid_calls(K, True):
        paths, logps = ref[W, layout]
        assert (tail == 255).all(), (K, W, b, s, layout)
        diff = int((path != paths[b][s]).sum())
        assert diff == 0, f"K={K} W={W} b={b} s={s} {layout}: {diff} of {len(path)} sites differ from the oracle's path"
        worst = max(worst, abs(logp / logps[b, s] - 1))
    print(f"PARITY viterbi K={K} f64: paths equal at every site, max rel logp error {worst:.3e}")
    assert worst < 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize("K", GRID_K)
def test_f32_path_is_almost_optimal(K):
    pp, pc, sets = grid_inputs(K)
    ref = {}
    for rows, W, lens in sets:
        ref[W, "bcast"] = oracle_grid(pp, rows, W, lens)
        ref[W, "chunk"] = oracle_grid(pc, rows, W, lens, per_chunk=True)
    worst_def, worst_lp, ndiff, nsite = 0.0, 0.0, 0, 0
    for q, b, s, row, W, path, tail, logp, layout in _grid_calls(K, False):
        paths, logps, _ = ref[W, layout]
        assert (tail == 255).all() and int(path.max()) < K
        assert _valid_path(q, path)
        deficit = logps[b, s] - vo.path_logp(q, row, path, W)
        assert deficit >= -1e-9 * abs(logps[b, s]), "a path above the optimum: the oracle or the scoring is wrong"
        exact = vo.deficit(q, row, paths[b][s], path, W)  # term by term: free of the rounding of the two sums
        assert exact >= 0.0
        worst_def = max(worst_def, deficit / len(row), exact / len(row))
        worst_lp = max(worst_lp, abs(logp / logps[b, s] - 1))
        ndiff += int((path != paths[b][s]).sum())
        nsite += len(path)
    print(f"PARITY viterbi K={K} f32: max deficit per site {worst_def:.3e}, max rel logp error {worst_lp:.3e}, "
          f"{ndiff} of {nsite} sites ({ndiff / nsite:.2%}) differ from the oracle's path")
    assert worst_def <= F32_VITERBI_DEFICIT_BAR, worst_def
    assert worst_lp < F32_LOGP_BAR, worst_lp


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [True, False])
def test_lens_is_the_row_cut_not_the_row_padded(dbl):
    from phlash_amd.kernel import get_kernel

    K, L, n = 16, 900, 611
    pp = _bcast(_population(K, 2, seed=5))
    wide = _rows(2, L, seed=8, het=0.05)
    lens = np.array([n, L])
    cut = np.ascontiguousarray(wide[:1, :n])
    for W in (0, 37):
        a = get_kernel(K, wide, double_precision=dbl, overlap=W).viterbi(pp, np.arange(2), lens=lens)
        c = get_kernel(K, cut, double_precision=dbl, overlap=W).viterbi(pp, np.arange(1))
        assert torch.equal(a.path[:, 0, : n - W], c.path[:, 0])
        assert bool((a.path[:, 0, n - W :] == 255).all()) and bool((a.path[:, 1] != 255).all())
        rel = float((a.logp[:, 0] / c.logp[:, 0] - 1).abs().max())
        assert rel < (1e-12 if dbl else 1e-6), rel
        # the same row padded with missing windows and no lens is another problem: allowed to differ
        padded = wide.copy()
        padded[0, n:] = -1
        p = get_kernel(K, padded, double_precision=dbl, overlap=W).viterbi(pp, np.arange(2))
        d = (p.path[:, 0, : n - W] != c.path[:, 0])
        first = [int(torch.nonzero(x)[0]) + W if bool(x.any()) else None for x in d]
        print(f"lens ({'f64' if dbl else 'f32'}, W={W}): padded with missing windows instead: {int(d.sum())} sites differ "
              f"(first at {first}), logp {p.logp[:, 0].tolist()} vs {c.logp[:, 0].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_identities_slabs_repeats_and_plans(dbl):
    from phlash_amd.kernel import get_kernel

    rows = _rows(4, 5000, seed=5, het=0.05, run=300)
    pop = _population(16, 3, seed=7)
    pp = _bcast(pop)
    inds = np.arange(4)
    # max <= sum at W = 0, for every sequence
    k0 = get_kernel(16, rows, double_precision=dbl, overlap=0)
    v0 = k0.viterbi(pp, inds)
    ll = k0.loglik(pp, inds)
    assert bool((v0.logp <= ll).all()), (v0.logp, ll)
    path = v0.path.cpu().numpy()
    for b in range(3):
        q = _pp_np(pop, b)
        for s in range(4):
            assert _valid_path(q, path[b, s])
    # a gradient call before and after: identical bits, plan untouched; repeats are bitwise equal; slabs change nothing
    kern = get_kernel(16, rows, double_precision=dbl, overlap=200)
    eng = kern._eng
    ll0, g0 = kern(pp, inds, grad=True)
    plan0 = eng.get_plan()
    a = kern.viterbi(pp, inds)
    b_ = kern.viterbi(pp, inds)
    assert torch.equal(a.path, b_.path) and torch.equal(a.logp, b_.logp)
    ll1, g1 = kern(pp, inds, grad=True)
    assert torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert eng.get_plan() == plan0
    eng.set_workspace_limit(1 << (18 if dbl else 17))  # three sequences per slab
    c = kern.viterbi(pp, inds)
    eng.set_workspace_limit(1 << 40)
    assert torch.equal(a.path, c.path) and torch.equal(a.logp, c.logp)
    assert a.path.shape == (3, 4, 4800)


@pytest.mark.gpu
def test_extreme_parameters_are_re_evaluated_with_per_site_rescaling():
    """Emissions so small on a run of het sites that four unscaled steps take the maximum below the float64 kernels' threshold
    (2^-600): the flag's normal path, as in test_hip_parity's extreme-emission test."""
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    K = 16
    pop = _population(K, 1, seed=0)
    q = _pp_np(pop, 0)
    q = q._replace(emis1=1e-46 * (1.0 + np.arange(K) / K), emis0=1.0 - 1e-46 * (1.0 + np.arange(K) / K))
    data = np.ones((1, 64), dtype=np.int8)
    data[0, 40:48] = 0
    path, logp, margin = vo.viterbi(q, data[0], 0)
    assert margin >= MIN_MARGIN, margin
    kern = get_kernel(K, data, double_precision=True)
    with pytest.warns(UserWarning, match="per-site rescaling"):
        out = kern.viterbi(PSMCParams(*(torch.as_tensor(x) for x in q)), np.int64(0))
    assert np.array_equal(out.path.cpu().numpy(), path)
    assert abs(float(out.logp) / logp - 1) < 1e-11


@pytest.mark.gpu
def test_one_row_of_3_000_001_windows():
    """The deficit is summed term by term (viterbi_oracle.deficit).  The oracle's own logp is a running float64 sum of
    3,000,001 terms of size 0.2: it ends 4.3e-7 (1.4e-13 per site) above the correctly rounded sum of the same terms, more
    than the bar, although the float32 path equals the oracle's at every site (measured on the MI355X; the float64 kernel's
    logp equals the correctly rounded sum to the last digit).  That difference is printed, not asserted."""
    from phlash_amd.engine import HipEngine

    L = 3_000_001
    rng = np.random.default_rng(9)
    data = (rng.random((1, L), dtype=np.float32) < 0.05).astype(np.int8)
    data.flat[rng.integers(0, L, L // 100)] = -1
    data[0, 0] = 1
    eng = HipEngine(16, data, double_precision=False)
    pop = _population(16, 1, seed=3)
    P = torch.stack(list(pop), -2)[:, None].cuda()
    inds = torch.zeros(1, dtype=torch.int64, device="cuda")
    logp, path = eng.viterbi(P, inds, 0)
    assert not eng.underflow_risk()
    assert path.shape == (1, 1, L) and bool(torch.isfinite(logp).all())
    z = path[0, 0].cpu().numpy()
    assert int(z.max()) < 16
    q = _pp_np(pop, 0)
    assert _valid_path(q, z)
    own = vo.path_logp(q, data[0], z, 0)
    rel = abs(float(logp) / own - 1)
    ref, best, _ = vo.viterbi(q, data[0], 0, want_margin=False)
    deficit = vo.deficit(q, data[0], ref, z, 0)
    print(f"3,000,001-window row: kernel logp vs float64 score of its own path rel {rel:.2e}; {int((z != ref).sum())} sites differ "
          f"from the oracle's path, deficit {deficit:.3e} ({deficit / L:.3e} per site); the oracle's running sum minus the score "
          f"of the kernel's path: {best - own:.3e}")
    assert rel < F32_LOGP_BAR
    assert best - own >= -1e-9 * abs(best)
    assert 0.0 <= deficit / L <= F32_VITERBI_DEFICIT_BAR


@pytest.mark.gpu
def test_recovers_the_simulated_path_and_decodes_ragged_contigs():
    import phlash_amd
    from phlash_amd.data import RawContig
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel
    from test_posterior_decode import simulate_with_path

    K = 16
    data, truth, dm = simulate_with_path(K, 4, 50_000, seed=21, theta=0.05, rho=0.05)
    kern = get_kernel(K, data, double_precision=False)
    out = kern.viterbi(dm, np.arange(4))
    z = out.path.cpu().numpy().astype(int)
    q = pn.PP(*(np.asarray(x, float) for x in PSMCParams.from_dm(dm)))
    ref = np.stack([vo.viterbi(q, data[s], 0, want_margin=False)[0] for s in range(4)]).astype(int)
    share_gpu = float((np.abs(z - truth) <= 1).mean())
    share_ref = float((np.abs(ref - truth) <= 1).mean())
    print(f"sites within one state of the simulated path: kernel {share_gpu:.4f}, float64 oracle {share_ref:.4f}; "
          f"kernel path differs from the oracle's at {float((z != ref).mean()):.2%} of sites")
    assert share_gpu >= share_ref - 0.01
    # viterbi_tmrca: rates per base pair; ragged contigs are decoded at their own lengths
    ws = 100
    dmb = DemographicModel(eta=dm.eta, theta=dm.theta / ws, rho=dm.rho / ws)
    path, track = phlash_amd.viterbi_tmrca(dmb, data, window_size=ws)
    assert path.shape == (4, 50_000) and path.dtype == torch.uint8 and track.dtype == torch.float64
    assert torch.equal(path, out.path)
    ect = torch.as_tensor(dm.eta.ect(), dtype=torch.float64, device=path.device)
    assert torch.equal(track, ect[path.long()])
    cs = [RawContig(data[:2, :30_000], np.ones(1), ws), RawContig(data[2:, :], np.ones(1), ws)]
    rp, rt = phlash_amd.viterbi_tmrca(dmb, cs, window_size=ws)
    assert [tuple(x.shape) for x in rp] == [(2, 30_000), (2, 50_000)] == [tuple(x.shape) for x in rt]
    alone_p, alone_t = phlash_amd.viterbi_tmrca(dmb, np.ascontiguousarray(data[:2, :30_000]), window_size=ws)
    assert torch.equal(rp[0], alone_p) and torch.equal(rt[0], alone_t)
    assert torch.equal(rp[1], path[2:])
    both_p, both_t = phlash_amd.viterbi_tmrca([dmb, dmb], data, window_size=ws)
    assert both_p.shape == (2, 4, 50_000) and torch.equal(both_p[0], path) and torch.equal(both_p[1], path)
    # the segment table re-expands to the path
    segs = phlash_amd.tmrca_segments(rp[0], values=ect)
    assert np.array_equal(_expand(segs, 2, 30_000), rp[0].cpu().numpy())
    assert torch.equal(segs[4], ect[segs[3]])
    assert bool((segs[2] > segs[1]).all())
