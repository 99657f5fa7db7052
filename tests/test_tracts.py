"""Tract posteriors (phk_tracts / HipEngine.tracts / PSMCKernel.tracts / phlash_amd.tract_posterior).

CPU: the float64 dense oracle against path enumeration (indicator and fractional weights, a missing site, a row's own length
inside a bin); the structured (loop-form) statement of the kernel's arithmetic against the dense oracle on the GPU grid's
inputs; the ABI's argument check without a device; the lazy re-export.
GPU: the tracts against the oracle for every compiled K (and a padded one) in both precisions with ragged lens and three
weight rows; the identities against shipped code (the marginals at bin = 1, m = 1, the likelihood ratio of the no-gradient
call, nested sets, a bin against its sites); ll bitwise phk_posterior's; plans / slabs / repeat calls; whole contigs of
different lengths; and the share of sampled paths that stay inside the set.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import tract_bars as bars
import tract_oracle as to
from test_posterior_decode import _bcast, _pp_np, _population, _random_pp, _rows, simulate_with_path

GRID_K = [4, 8, 12, 16, 32, 64]
GRID_B, GRID_S, GRID_L = 2, 3, 700
GRID_BINS = (1, 7, 100)
GRID_WEIGHTS = ("prefix", "interior", "fractional")


# ------------------------------------------------------------------------------------------------- shared inputs
def grid_sets():
    """The two row sets of the oracle grid: (rows, W, lens), those of the predictive grid.  Rows with isolated missing sites
    (both) and with runs of 120 missing windows (the second).  lens: 593 and 437 end inside a block (of 8 and of 16 sites) and
    inside a bin of 7; 300 (W = 0) and 437 (W = 37) leave whole bins of 100 without a site of the row's own; 655 ends inside a
    bin of 100.  The first set keeps its data past the own lengths (the mask alone), row 0 of the second is padded with missing
    windows past its own length."""
    r1 = _rows(GRID_S, GRID_L, seed=1)
    r2 = _rows(GRID_S, GRID_L, seed=2, run=120)
    r2[0, 437:] = -1
    return [(r1, 0, np.array([700, 593, 300])), (r2, 37, np.array([437, 700, 655]))]


def grid_weights(K):
    """-> {name: [B, K] or [K]}: a prefix set (the states below 5K/8 + b: one more for the second particle), an interior set
    (K/4 <= k < 3K/4 + b) and fractional weights in (0.9, 1] (one row for all particles: the stride-0 form)."""
    k = np.arange(K)
    rng = np.random.default_rng(50 + K)
    w = {
        "prefix": np.stack([(k < (5 * K) // 8 + b).astype(float) for b in range(GRID_B)]),
        "interior": np.stack([((k >= K // 4) & (k < (3 * K) // 4 + b)).astype(float) for b in range(GRID_B)]),
        "fractional": 1.0 - 0.1 * rng.random(K),
    }
    for a in w.values():
        a.setflags(write=False)
    return w


def _rows_of(w, b):
    """the three weight rows of particle b, [3, K]"""
    return np.stack([w[n] if w[n].ndim == 1 else w[n][b] for n in GRID_WEIGHTS])


@functools.lru_cache(maxsize=None)
def grid_oracle(K):
    """-> {(set, layout): ({bin: tract [3 weights, B, S, nbin]}, ll [B, S])} of the dense float64 oracle, once per K"""
    pp = _population(K, GRID_B, seed=K)
    pc = _population(K, GRID_B * GRID_S, seed=1000 + K)  # one model per (particle, chunk), all different
    w = grid_weights(K)
    out = {}
    for i, (rows, W, lens) in enumerate(grid_sets()):
        for layout in ("bcast", "chunk"):
            T = {bin: np.zeros((3, GRID_B, GRID_S, (GRID_L - W + bin - 1) // bin)) for bin in GRID_BINS}
            ll = np.empty((GRID_B, GRID_S))
            for b in range(GRID_B):
                for s in range(GRID_S):
                    q = _pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * GRID_S + s)
                    tr, ll[b, s] = to.dense(q, rows[s], _rows_of(w, b), W, GRID_BINS, int(lens[s]))
                    for bin, t in zip(GRID_BINS, tr):
                        T[bin][:, b, s] = t
            for t in T.values():
                t.setflags(write=False)
            out[i, layout] = (T, ll)
    return out


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K,L,W,bin", [(2, 8, 0, 3), (3, 7, 1, 3), (4, 6, 0, 1), (4, 6, 1, 3), (3, 8, 1, 1)])
def test_oracle_against_path_enumeration(K, L, W, bin):
    rng = np.random.default_rng(K * 100 + L * 10 + W + bin)
    pp = _random_pp(K, rng)
    data = rng.integers(-1, 2, size=L)
    data[0] = 1  # a het at site 0
    data[L // 2] = -1  # a missing site mid-row
    ind = (np.arange(K) < max(1, K // 2)).astype(float)  # an indicator
    frac = rng.random(K)  # fractional weights
    length = W + bin + 1 if bin > 1 else L - 2  # ends inside the second bin / leaves bins without a site of the row's own
    for m in (ind, frac):
        for n in (None, length):
            t, ll = to.dense(pp, data, m, W, bin, n)
            tb = to.bruteforce(pp, data, m, W, bin, n)
            assert t.shape == tb.shape == ((L - W + bin - 1) // bin,)
            np.testing.assert_allclose(t, tb, rtol=0, atol=1e-15)
            assert (t >= 0).all() and (t <= 1 + 1e-15).all()
            if n is not None:
                assert not t[(n - W + bin - 1) // bin :].any() and t[: (n - W + bin - 1) // bin].all()
    # several weight rows and bin sizes in one pass are the single calls
    many, _ = to.dense(pp, data, np.stack([ind, frac]), W, (1, bin), length)
    for g, bn in enumerate((1, bin)):
        for j, m in enumerate((ind, frac)):
            np.testing.assert_allclose(many[g][j], to.dense(pp, data, m, W, bn, length)[0], rtol=0, atol=1e-15)  # (the matrix products' shapes differ)
    import posterior_oracle as po

    _, llb = po.bruteforce(pp, data, W)
    assert abs(ll - llb) < 1e-12 * abs(llb) + 1e-13


def test_oracle_one_bin_is_a_likelihood_ratio():
    """one bin over a whole row without missing sites: log tract = ll(emis0, emis1 multiplied by m) - ll"""
    import posterior_oracle as po

    rng = np.random.default_rng(3)
    K, L = 8, 120
    pp = _random_pp(K, rng)
    data = (rng.random(L) < 0.1).astype(int)
    m = 1.0 - 0.2 * rng.random(K)
    t, ll = to.dense(pp, data, m, 0, L)
    _, ll0 = po.forward_backward(pp, data, 0)
    _, ll1 = po.forward_backward(pp._replace(emis0=pp.emis0 * m, emis1=pp.emis1 * m), data, 0)
    assert t.shape == (1,) and abs(ll - ll0) < 1e-12 * abs(ll0)
    assert abs(np.log(t[0]) - (ll1 - ll0)) < 1e-12 * abs(ll1 - ll0)


@functools.lru_cache(maxsize=None)
def structured_floor(K):
    """the structured float64 statement against the dense oracle on the GPU grid's inputs (every particle and row of both sets
    in both parameter layouts, the grid's weights, bins and lens), in the GPU grid's own metric: the largest absolute error"""
    pp = _population(K, GRID_B, seed=K)
    pc = _population(K, GRID_B * GRID_S, seed=1000 + K)
    w = grid_weights(K)
    worst = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        for layout in ("bcast", "chunk"):
            T, _ = grid_oracle(K)[i, layout]
            for b in range(GRID_B):
                for s in range(GRID_S):
                    q = _pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * GRID_S + s)
                    tr = to.structured(q, rows[s], _rows_of(w, b), W, GRID_BINS, int(lens[s]))
                    for bin, t in zip(GRID_BINS, tr):
                        worst = max(worst, float(np.abs(t - T[bin][:, b, s]).max()))
    return worst


@pytest.mark.parametrize("K", GRID_K)
def test_structured_statement_against_the_dense_oracle(K):
    """The kernel's form in float64 loops (folded factors, the adjoint mat-vec's running sums, one power-of-two rescale shared
    by beta and q) against the dense oracle: the float64 rounding floor the GPU bars are judged against
    (tract_bars.STRUCTURED_FLOOR)."""
    worst = structured_floor(K)
    print(f"PARITY tracts structured-vs-dense K={K}: max |tract - oracle| = {worst:.3e}")
    assert worst < bars.STRUCTURED_FLOOR_BAR, worst


def test_float64_bars_are_within_ten_floors():
    assert bars.F64_TRACT_BAR <= 10 * bars.STRUCTURED_FLOOR


def test_phk_tracts_rejects_a_null_handle_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_tracts" in _lib.SIGNATURES
    rc = lib.phk_tracts(None, None, 0, 0, None, None, 1, 1, 0, 1, None, 0, None, None, None, None)
    assert rc == _lib.PHK_EINVAL
    assert b"NULL" in lib.phk_last_error()


def test_tract_posterior_is_lazy_and_has_no_cpu_fallback(monkeypatch):
    import phlash_amd

    f = phlash_amd.tract_posterior
    from phlash_amd.decode import tract_posterior

    assert f is tract_posterior
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dm = phlash_amd.DemographicModel.default("4*1", 1e-4, 1e-4)
    data = np.zeros((1, 50), dtype=np.int8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        tract_posterior(dm, data, t_max=1.0)


SMP_K, SMP_ROWS, SMP_SITES, SMP_BIN, SMP_N, SMP_DATA_SEED, SMP_SEED, SMP_PREFIX = 16, 2, 600, 50, 4000, 21, 11, 9


@functools.lru_cache(maxsize=None)
def sampled():
    """-> (data, dm, the weight row of the prefix set, the float64 oracle's tract [rows, nbin]) of the path-sampling test.  The
    data seed and the set (the SMP_PREFIX youngest states) were chosen on the CPU with the oracle so that enough bins have a
    probability away from 0 and 1 (test_sampling_case_has_enough_bins)."""
    from phlash_amd.params import PSMCParams

    data, _, dm = simulate_with_path(SMP_K, SMP_ROWS, SMP_SITES, seed=SMP_DATA_SEED, theta=0.05, rho=0.05)
    m = (np.arange(SMP_K) < SMP_PREFIX).astype(float)
    pp = PSMCParams.from_dm(dm)
    q = _pp_np(PSMCParams(*(torch.as_tensor(a)[None] for a in pp)), 0)
    p = np.stack([to.dense(q, data[s], m, 0, SMP_BIN)[0] for s in range(SMP_ROWS)])
    return data, dm, m, p


def test_sampling_case_has_enough_bins():
    _, _, _, p = sampled()
    ok = SMP_N * p * (1 - p) >= 25
    print(f"path-sampling case: oracle tracts {np.round(p, 4).tolist()}, {int(ok.sum())} of {p.size} bins qualify")
    assert p.shape == (SMP_ROWS, SMP_SITES // SMP_BIN) and p.size == 24
    assert ok.sum() >= 8


# ------------------------------------------------------------------------------------------------- GPU
def _np(x):
    return x.double().cpu().numpy()


def _chunk(pc, B, S, K):
    from phlash_amd.params import PSMCParams

    return PSMCParams(*(torch.as_tensor(a).reshape(B, S, K).contiguous() for a in pc))


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
@pytest.mark.parametrize("K", GRID_K)
def test_tracts_against_the_oracle(K, dbl):
    from phlash_amd.kernel import get_kernel

    B, S = GRID_B, GRID_S
    pp = _population(K, B, seed=K)
    pc = _population(K, B * S, seed=1000 + K)
    w = grid_weights(K)
    worst = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        for layout in ("bcast", "chunk"):
            T, LL = grid_oracle(K)[i, layout]
            q = _bcast(pp) if layout == "bcast" else _chunk(pc, B, S, K)
            for bin in GRID_BINS:
                n = GRID_L - W
                empty = np.array([[min((k + 1) * bin, n, int(lens[s]) - W) <= k * bin for k in range(T[bin].shape[-1])] for s in range(S)])
                assert empty.any()
                for j, name in enumerate(GRID_WEIGHTS):
                    out = kern.tracts(q, np.arange(S), weights=w[name], bin=bin, lens=lens)
                    t = _np(out.prob)
                    assert t.shape == T[bin][j].shape
                    assert np.isfinite(t).all() and (t >= 0).all() and (t <= 1).all()
                    worst = max(worst, float(np.abs(t - T[bin][j]).max()))
                    # a bin without a site of the row's own is 0, exactly; every other bin of these rows is positive
                    assert not t[:, empty].any() and not T[bin][j][:, empty].any()
                    assert (T[bin][j][:, ~empty] > 0).all()
                    rel = np.abs(out.ll.cpu().numpy() / LL - 1).max()
                    assert rel < (1e-12 if dbl else 1e-5), (bin, layout, W, rel)
    print(f"PARITY tracts K={K} {'f64' if dbl else 'f32'}: max |tract - oracle| = {worst:.3e}")
    assert worst < (bars.F64_TRACT_BAR if dbl else bars.F32_TRACT_BAR), worst
    if dbl:
        assert bars.F64_TRACT_BAR <= 10 * bars.STRUCTURED_FLOOR


def _kernel16(dbl=False, S=4, L=5000, W=200, seed=5):
    from phlash_amd.kernel import get_kernel

    rows = _rows(S, L, seed=seed, het=0.05, run=300)
    return rows, get_kernel(16, rows, double_precision=dbl, overlap=W)


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_single_sites_are_phk_posteriors_marginals(dbl):
    """bin = 1: the tract of one site is sum_k m(k) gamma_t(k)"""
    rows, kern = _kernel16(dbl)
    q = _population(16, 3, seed=2)
    pp = _bcast(q)
    inds = np.arange(4)
    g = kern.posterior(pp, inds, bin=1).marginals.double()  # [B, S, n, K]
    worst = 0.0
    for name, m in grid_weights(16).items():
        m = m if m.ndim == 1 else np.concatenate([m, m[:1]])  # (three particles here: a row each)
        out = kern.tracts(pp, inds, weights=m, bin=1)
        mt = torch.tensor(m, dtype=torch.float64, device=g.device)
        ref = (g * (mt[:, None, None, :] if mt.ndim == 2 else mt)).sum(-1)
        assert torch.isfinite(out.prob).all()
        err = float((out.prob.double() - ref).abs().max())
        print(f"tract at bin = 1 vs marginals ({'f64' if dbl else 'f32'}, {name}): max |diff| {err:.2e}")
        worst = max(worst, err)
    print(f"PARITY tracts marginal identity {'f64' if dbl else 'f32'}: max |diff| = {worst:.3e}")
    assert worst < (bars.F64_MARGINAL_BAR if dbl else bars.F32_MARGINAL_BAR), worst


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_unit_weights_give_one_and_empty_bins_zero(dbl):
    """m = 1: q is beta bit for bit (the same operations on the same numbers), so the ratio is exactly 1"""
    rows, kern = _kernel16(dbl)
    pp = _bcast(_population(16, 3, seed=2))
    lens = np.array([5000, 4321, 5000, 777])
    W = kern.overlap
    for bin in (1, 7, 600):
        t = _np(kern.tracts(pp, np.arange(4), weights=np.ones(16), bin=bin, lens=lens).prob)
        n = 5000 - W
        empty = np.array([[min((k + 1) * bin, n, int(lens[s]) - W) <= k * bin for k in range(t.shape[-1])] for s in range(4)])
        assert empty.any()
        print(f"m = 1, bin {bin} ({'f64' if dbl else 'f32'}): max |tract - 1| = {np.abs(t[:, ~empty] - 1).max():.2e}")
        assert (t[:, ~empty] == 1).all() and not t[:, empty].any()


@pytest.mark.gpu
def test_one_bin_is_the_likelihood_ratio_of_loglik():
    """One bin of L sites, W = 0, a row without missing sites, strictly positive fractional m, float64, K = 16:
    log tract = ll(emis0, emis1 multiplied by m) - ll, both from the shipped no-gradient call: code that shares only the forward
    step with the tract sweep."""
    from phlash_amd.kernel import get_kernel

    L = 200
    rng = np.random.default_rng(17)
    data = (rng.random((2, L)) < 0.05).astype(np.int8)
    data[:, 0] = 1
    kern = get_kernel(16, data, double_precision=True, overlap=0)
    q = _population(16, 2, seed=4)
    m = 1.0 - 0.1 * rng.random((2, 16))
    out = kern.tracts(_bcast(q), np.arange(2), weights=m, bin=L)
    assert out.prob.shape == (2, 2, 1)
    lt = np.log(_np(out.prob)[..., 0])
    qm = q._replace(emis0=torch.as_tensor(q.emis0) * torch.as_tensor(m), emis1=torch.as_tensor(q.emis1) * torch.as_tensor(m))
    ll0 = np.asarray(kern(_bcast(q), np.arange(2), grad=False).cpu().numpy(), float)
    ll1 = np.asarray(kern(_bcast(qm), np.arange(2), grad=False).cpu().numpy(), float)
    err = np.abs(lt - (ll1 - ll0)).max()
    print(f"log tract {lt.tolist()}, ll ratio {(ll1 - ll0).tolist()}")
    print(f"PARITY tracts likelihood-ratio identity: max |log tract - (ll_m - ll)| = {err:.3e}")
    assert (lt < -1).all()  # (a ratio far from 1: the identity says something)
    assert bars.F64_LIKELIHOOD_RATIO_BAR < 1e-10
    assert err < bars.F64_LIKELIHOOD_RATIO_BAR, err


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_nested_sets_and_bins_against_their_sites(dbl):
    rows, kern = _kernel16(dbl)
    pp = _bcast(_population(16, 3, seed=2))
    inds = np.arange(4)
    k = np.arange(16)
    small, large = ((k >= 3) & (k < 9)).astype(float), ((k >= 2) & (k < 11)).astype(float)
    # a set inside another: q <= q' elementwise in the computed numbers (every operation is monotone), so no tolerance
    for bin in (1, 7, 100):
        a = _np(kern.tracts(pp, inds, weights=small, bin=bin).prob)
        b = _np(kern.tracts(pp, inds, weights=large, bin=bin).prob)
        assert (a <= b).all() and (b <= 1).all() and (a < b).any()
    # a bin against each of its sites: P(all sites in S) <= P(site t in S)
    tol = bars.F64_TRACT_BAR if dbl else bars.F32_TRACT_BAR
    one = _np(kern.tracts(pp, inds, weights=large, bin=1).prob)
    n = one.shape[-1]
    for bin in (7, 100):
        t = _np(kern.tracts(pp, inds, weights=large, bin=bin).prob)
        nb = t.shape[-1]
        pad = np.full(one.shape[:-1] + (nb * bin,), np.inf)
        pad[..., :n] = one
        low = pad.reshape(one.shape[:-1] + (nb, bin)).min(-1)
        print(f"bin {bin} ({'f64' if dbl else 'f32'}): max (tract - min of its sites) = {(t - low).max():.2e}")
        assert (t <= low + tol).all()


@pytest.mark.gpu
def test_ll_is_bitwise_phk_posteriors():
    rows, kern = _kernel16(False)
    pp = _bcast(_population(16, 3, seed=2))
    inds = np.arange(4)
    m = grid_weights(16)["fractional"]
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        kern._eng.set_plan(*plan)
        a = kern.tracts(pp, inds, weights=m, bin=7).ll
        b = kern.posterior(pp, inds, bin=7).ll
        assert torch.equal(a, b), (plan, float((a - b).abs().max()))


@pytest.mark.gpu
def test_plans_slabs_and_repeats_are_consistent():
    rows, kern = _kernel16(False)
    eng = kern._eng
    pp = _bcast(_population(16, 3, seed=7))
    inds = np.arange(4)
    lens = np.array([5000, 4321, 5000, 777])
    k = np.arange(16)
    m = np.stack([(k < 8 + b).astype(float) for b in range(3)])  # a row per particle: slabs must offset it
    same = lambda x, y: all(torch.equal(p, q) for p, q in zip(x, y))  # noqa: E731
    ll0, g0 = kern(pp, inds, grad=True)  # the gradient call before any tract call
    plan0 = eng.get_plan()
    a = kern.tracts(pp, inds, weights=m, bin=7, lens=lens)
    b = kern.tracts(pp, inds, weights=m, bin=7, lens=lens)
    assert same(a, b)
    ll1, g1 = kern(pp, inds, grad=True)
    assert torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert eng.get_plan() == plan0
    # bins: 7 straddles block, segment and unit edges; 600 is larger than a segment of 512 sites; W = 200 lies inside a block
    # of 16 sites (the segmented plan's)
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        for bin in (7, 600):
            eng.set_plan(*plan)  # (a slab is a launch shape of its own: fix the plan so that both runs use the same one)
            a = kern.tracts(pp, inds, weights=m, bin=bin, lens=lens)
            eng.set_workspace_limit(1 << 17)  # three sequences per slab
            c = kern.tracts(pp, inds, weights=m, bin=bin, lens=lens)
            eng.set_workspace_limit(1 << 40)
            assert same(a, c), (plan, bin)
    for bin in (7, 600):
        eng.set_plan(0, 4, 8, 4, 0)
        ser = _np(kern.tracts(pp, inds, weights=m, bin=bin, lens=lens).prob)
        eng.set_plan(1, 4, 16, 4, 4)
        assert eng.get_plan()["segmented"] == 1
        seg = _np(kern.tracts(pp, inds, weights=m, bin=bin, lens=lens).prob)
        err = np.abs(seg - ser).max()
        print(f"serial vs segmented plan, bin {bin}: max |diff| {err:.2e}")
        assert err < bars.F32_TRACT_BAR


@pytest.mark.gpu
def test_whole_contigs_padding_changes_nothing():
    import phlash_amd
    from phlash_amd.size_history import DemographicModel

    data, dm, _, _ = sampled()
    ws, bin = 100, 10
    dms = [DemographicModel(eta=dm.eta, theta=dm.theta / ws, rho=dm.rho / ws),
           DemographicModel(eta=dm.eta._replace(c=dm.eta.c * 1.5), theta=dm.theta / ws, rho=dm.rho / ws)]
    t_max = float(dm.eta.t[SMP_PREFIX])  # the SMP_PREFIX youngest states
    contigs = [data[:1, :345], data[1:, :]]  # 345 windows end inside a bin of 10 and inside a block
    rag = phlash_amd.tract_posterior(dms[0], contigs, t_max, window_size=ws, bin=bin)
    assert [tuple(r.shape) for r in rag] == [(1, 35), (1, 60)] and rag[0].dtype == torch.float64
    for c, r in zip(contigs, rag):
        alone = phlash_amd.tract_posterior(dms[0], c, t_max, window_size=ws, bin=bin)
        err = float((r - alone).abs().max())
        print(f"contig of {c.shape[1]} windows, padded vs alone: max |diff| {err:.2e}")
        assert err < bars.F32_TRACT_BAR
        assert float(r.min()) >= 0 and float(r.max()) <= 1 and float(r.max()) > 0
    # the range is the set: the explicit weights of the same states, and the kernel's own call
    m = (np.arange(SMP_K) < SMP_PREFIX).astype(float)
    both = phlash_amd.tract_posterior(dms, data, t_max, window_size=ws, bin=bin)
    each = [phlash_amd.tract_posterior(d, data, 0.0, window_size=ws, bin=bin, weights=m) for d in dms]
    assert both.shape == (SMP_ROWS, SMP_SITES // bin) and both.dtype == torch.float64
    assert float((both - (each[0] + each[1]) / 2).abs().max()) < 1e-12
    # an interior range drops the youngest state and the open last one
    inner = phlash_amd.tract_posterior(dms[0], data, t_max, t_min=float(dm.eta.t[1]), window_size=ws, bin=bin)
    ref = phlash_amd.tract_posterior(dms[0], data, 0.0, window_size=ws, bin=bin, weights=m * (np.arange(SMP_K) >= 1))
    assert torch.equal(inner, ref)
    whole = phlash_amd.tract_posterior(dms[0], data, np.inf, window_size=ws, bin=bin)
    assert bool((whole == 1).all())


@pytest.mark.gpu
def test_sampled_paths_stay_in_the_set_as_often_as_the_tract_says():
    """K = 16 float32, one model, 2 rows x 600 windows, bin = 50, 4,000 draws, a prefix set: for every bin with n p (1 - p) >= 25
    (p the float64 oracle's), |share of draws whose whole bin stays in S - kernel tract| <= 5 sqrt(p (1 - p) / n)."""
    from phlash_amd.kernel import get_kernel

    data, dm, m, p = sampled()
    kern = get_kernel(SMP_K, data, double_precision=False)
    inds = np.arange(SMP_ROWS)
    t = _np(kern.tracts(dm, inds, weights=m, bin=SMP_BIN).prob)  # [rows, nbin]
    paths = kern.sample_paths(dm, inds, n_samples=SMP_N, seed=SMP_SEED).paths  # [rows, n, L] uint8
    assert paths.shape == (SMP_ROWS, SMP_N, SMP_SITES)
    inside = torch.as_tensor(m > 0, device=paths.device)[paths.long()]
    share = _np(inside.reshape(SMP_ROWS, SMP_N, SMP_SITES // SMP_BIN, SMP_BIN).all(-1).double().mean(1))
    ok = SMP_N * p * (1 - p) >= 25
    assert ok.sum() >= 8
    z = np.abs(share - t) / np.sqrt(p * (1 - p) / SMP_N)
    print(f"qualifying bins {int(ok.sum())} of {p.size}; kernel tract {np.round(t[ok], 4).tolist()}; share of draws "
          f"{np.round(share[ok], 4).tolist()}; worst |share - tract| in standard errors {z[ok].max():.2f}")
    assert np.abs(t - p).max() < bars.F32_TRACT_BAR
    assert (z[ok] <= 5).all(), z[ok]
