"""Transition posteriors (phk_transitions / HipEngine.transitions / PSMCKernel.transitions / phlash_amd.posterior_changes).

CPU: the float64 dense oracle against path enumeration and against the forward-backward marginals, the structured (loop-form)
statement of the kernel's products against the dense oracle on the GPU grid's inputs, the ABI's argument check without a
device, the lazy re-export, and the simulated rows' own count of state changes against the oracle's expectation.
GPU: arrivals and changes against the oracle for every compiled K (and a padded one) in both precisions with ragged lens,
the identity that ties the sweep to the shipped gradient call, the marginals of phk_posterior, plans / slabs / repeat
calls, whole contigs of different lengths, and the expected number of changes against a simulated path's own.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import posterior_oracle as po
import transition_bars as bars
import transition_oracle as to
from test_posterior_decode import F32_GAMMA_BAR, F64_GAMMA_BAR, _bcast, _pp_np, _population, _random_pp, _rows, simulate_with_path

GRID_K = [4, 8, 12, 16, 32, 64]
GRID_B, GRID_S, GRID_L = 2, 3, 700


# ------------------------------------------------------------------------------------------------- shared inputs
def grid_sets():
    """The two row sets of the oracle grid: (rows, W, lens).  Rows with isolated missing sites (both) and with runs of missing
    windows (the second).  lens: 593 and 437 end inside a block (of 8 and of 16 sites) and inside a bin of 7; 300 (W = 0) and
    437 (W = 37) leave whole bins of 100 without a site of the row's own; 655 ends inside a bin of 100.  The first set keeps its
    data past the own lengths (the mask alone), row 0 of the second is padded with missing windows past its own length."""
    r1 = _rows(GRID_S, GRID_L, seed=1)
    r2 = _rows(GRID_S, GRID_L, seed=2, run=120)
    r2[0, 437:] = -1
    return [(r1, 0, np.array([700, 593, 300])), (r2, 37, np.array([437, 700, 655]))]


@functools.lru_cache(maxsize=None)
def grid_oracle(K):
    """-> {(set, layout): (arr [B, S, L - W, 3, K] per site, ll [B, S])} of the dense float64 oracle, computed once per K"""
    pp = _population(K, GRID_B, seed=K)
    pc = _population(K, GRID_B * GRID_S, seed=1000 + K)  # one model per (particle, chunk), all different
    out = {}
    for i, (rows, W, _) in enumerate(grid_sets()):
        for layout in ("bcast", "chunk"):
            arr = np.empty((GRID_B, GRID_S, GRID_L - W, 3, K))
            ll = np.empty((GRID_B, GRID_S))
            for b in range(GRID_B):
                for s in range(GRID_S):
                    q = _pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * GRID_S + s)
                    xi, ll[b, s] = to.pair_posteriors(q, rows[s], W)
                    arr[b, s] = to.arrivals_of(xi)
            arr.setflags(write=False)
            out[i, layout] = (arr, ll)
    return out


def _binned(arr, W, bin, lens):
    """per-site oracle [B, S, n, 3, K] -> (arrivals [B, S, nbin, 3, K], changes [B, S, nbin, 2])"""
    A, C = [], []
    for b in range(arr.shape[0]):
        ra, rc = zip(*(to.reduce_bins(arr[b, s], W, bin, None if lens is None else int(lens[s])) for s in range(arr.shape[1])))
        A.append(ra)
        C.append(rc)
    return np.array(A), np.array(C)


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K,L,W", [(2, 6, 0), (3, 6, 2), (4, 5, 0), (4, 5, 3)])
def test_oracle_against_path_enumeration(K, L, W):
    rng = np.random.default_rng(K * 10 + L + W)
    pp = _random_pp(K, rng)
    data = rng.integers(-1, 2, size=L)
    data[0] = 1
    data[L // 2] = -1  # a missing site
    xi, ll = to.pair_posteriors(pp, data, W)
    xb = to.bruteforce_pairs(pp, data, W)
    assert xi.shape == (L - W, K, K)
    np.testing.assert_allclose(xi, xb, rtol=0, atol=1e-13)
    _, llb = po.bruteforce(pp, data, W)
    assert abs(ll - llb) < 1e-12 * abs(llb) + 1e-13
    # the arrivals and the masked, binned reduction, from the enumeration's xi by hand
    arr = to.arrivals_of(xi)
    for t in range(L - W):
        for k in range(K):
            assert abs(arr[t, 0, k] - xb[t, k, k]) < 1e-13
            assert abs(arr[t, 1, k] - sum(xb[t, i, k] for i in range(k))) < 1e-13
            assert abs(arr[t, 2, k] - sum(xb[t, i, k] for i in range(k + 1, K))) < 1e-13
    length = L - 1
    A, C = to.reduce_bins(arr, W, 2, length)
    n_own = length - W
    assert A.shape == ((L - W + 1) // 2, 3, K) and C.shape == ((L - W + 1) // 2, 2)
    assert abs(C.sum() - sum(xb[t, i, j] for t in range(n_own) for i in range(K) for j in range(K) if i != j)) < 1e-12
    last = (n_own - 1) // 2
    np.testing.assert_allclose(A[last], arr[2 * last : n_own].mean(0), atol=1e-14)
    assert not A[last + 1 :].any() and not C[last + 1 :].any()


def test_oracle_against_marginals():
    rng = np.random.default_rng(5)
    for K, W in ((8, 0), (16, 40)):
        pp = _random_pp(K, rng)
        data = (rng.random(300) < 0.05).astype(int)
        data[rng.integers(0, 300, 5)] = -1
        data[100:130] = -1
        xi, ll = to.pair_posteriors(pp, data, W)
        g, llg = po.forward_backward(pp, data, W)
        np.testing.assert_allclose(to.arrivals_of(xi).sum(1), g, rtol=0, atol=1e-13)
        assert abs(ll - llg) < 1e-12 * abs(llg)


@pytest.mark.parametrize("K", GRID_K)
def test_structured_statement_against_the_dense_oracle(K):
    """The kernel's form in float64 loops (folded factors, exclusive prefix / suffix, per-site Z_t) against the dense oracle on
    the GPU grid's inputs (particle 0 of the broadcast layout, every row of both sets).  Measured: 7.4e-15 at worst (K = 16):
    the float64 rounding floor the GPU bars are judged against."""
    pp = _population(K, GRID_B, seed=K)
    worst = 0.0
    for i, (rows, W, _) in enumerate(grid_sets()):
        arr, _ = grid_oracle(K)[i, "bcast"]
        for s in range(GRID_S):
            worst = max(worst, np.abs(to.structured(_pp_np(pp, 0), rows[s], W) - arr[0, s]).max())
    print(f"PARITY transitions structured-vs-dense K={K}: max |diff| = {worst:.3e}")
    assert worst < bars.STRUCTURED_FLOOR_BAR, worst


def test_phk_transitions_rejects_a_null_handle_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_transitions" in _lib.SIGNATURES
    rc = lib.phk_transitions(None, None, 0, 0, None, None, 1, 1, 0, 1, None, None, None, None, None)
    assert rc == _lib.PHK_EINVAL
    assert b"NULL" in lib.phk_last_error()


def test_posterior_changes_is_lazy_and_has_no_cpu_fallback(monkeypatch):
    import phlash_amd

    f = phlash_amd.posterior_changes
    from phlash_amd.decode import posterior_changes

    assert f is posterior_changes
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dm = phlash_amd.DemographicModel.default("4*1", 1e-4, 1e-4)
    data = np.zeros((1, 50), dtype=np.int8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        posterior_changes(dm, data)


SIM_K, SIM_ROWS, SIM_SITES, SIM_SEED = 16, 2, 4000, 21


@functools.lru_cache(maxsize=None)
def simulated():
    """-> (data, dm, the path's own count of state changes over sites 1 .. L-1 per row, the oracle's expectation of it, its
    standard error from the oracle's per-site change probabilities treated as independent)"""
    from phlash_amd.params import PSMCParams

    data, path, dm = simulate_with_path(SIM_K, SIM_ROWS, SIM_SITES, seed=SIM_SEED, theta=0.05, rho=0.05)
    pp = PSMCParams.from_dm(dm)
    q = _pp_np(PSMCParams(*(torch.as_tensor(a)[None] for a in pp)), 0)
    own = (path[:, 1:] != path[:, :-1]).sum(1)
    exp, se = np.empty(SIM_ROWS), np.empty(SIM_ROWS)
    for s in range(SIM_ROWS):
        arr = to.arrivals_of(to.pair_posteriors(q, data[s], 0)[0])
        p = arr[1:, 1:].sum((1, 2))  # P(z_{t-1} != z_t | o), t = 1 .. L-1 (z_0, before site 0, is not part of the path)
        exp[s], se[s] = p.sum(), np.sqrt((p * (1 - p)).sum())
    return data, dm, own, exp, se


def test_simulated_seed_lies_inside_the_bar():
    _, _, own, exp, se = simulated()
    print(f"simulated rows: own changes {own}, oracle's expectation {exp}, standard error {se}")
    assert (own > 50).all()
    assert (np.abs(own - exp) < 6 * se).all(), (own, exp, se)


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
@pytest.mark.parametrize("K", GRID_K)
def test_transitions_against_the_oracle(K, dbl):
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    B, S = GRID_B, GRID_S
    pp = _population(K, B, seed=K)
    pc = _population(K, B * S, seed=1000 + K)
    worst_a = worst_c = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        for layout in ("bcast", "chunk"):
            arr, LL = grid_oracle(K)[i, layout]
            q = _bcast(pp) if layout == "bcast" else PSMCParams(*(torch.as_tensor(a).reshape(B, S, K).contiguous() for a in pc))
            for bin in (1, 7, 100):
                A, C = _binned(arr, W, bin, lens)
                out = kern.transitions(q, np.arange(S), bin=bin, lens=lens)
                a = out.arrivals.double().cpu().numpy()
                c = out.changes.double().cpu().numpy()
                assert a.shape == A.shape and c.shape == C.shape
                assert np.isfinite(a).all() and np.isfinite(c).all()
                worst_a = max(worst_a, np.abs(a - A).max())
                worst_c = max(worst_c, (np.abs(c - C) / np.maximum(1.0, C)).max())
                # a bin without a site of the row's own is zeros, exactly
                empty = ~(A.any(axis=(-1, -2)))
                assert not a[empty].any() and not c[empty].any()
                rel = np.abs(out.ll.cpu().numpy() / LL - 1).max()
                assert rel < (1e-12 if dbl else 1e-5), (bin, layout, W, rel)
    print(f"PARITY transitions K={K} {'f64' if dbl else 'f32'}: max |arrivals - oracle| = {worst_a:.3e}, "
          f"max |changes - oracle| / max(1, oracle) = {worst_c:.3e}")
    assert worst_a < (bars.F64_ARRIVALS_BAR if dbl else bars.F32_ARRIVALS_BAR), worst_a
    assert worst_c < (bars.F64_CHANGES_BAR if dbl else bars.F32_CHANGES_BAR), worst_c


@pytest.mark.gpu
def test_row_sums_match_the_gradient_call():
    """At W = 0 with one bin of L sites, L * arrivals = sum over the sites of (stay, up, down) = the theta * d ll / d theta rows
    of d, v and b: the transition mass the shipped gradient sweep books (code that shares only the forward step with the
    transition sweep)."""
    from phlash_amd.kernel import get_kernel

    L = 3000
    rows = _rows(3, L, seed=11, het=0.04)
    kern = get_kernel(16, rows, double_precision=True, overlap=0)
    q = _bcast(_population(16, 2, seed=4))
    arr = kern.transitions(q, np.arange(3), bin=L).arrivals.double().cpu().numpy()  # [B, S, 1, 3, K]
    assert arr.shape == (2, 3, 1, 3, 16)
    _, dll = kern(q, np.arange(3), grad=True)
    worst = 0.0
    for j, name in enumerate(("d", "v", "b")):
        g = getattr(dll, name)
        g = np.asarray(g.cpu().numpy() if isinstance(g, torch.Tensor) else g, float)
        err = np.abs(L * arr[:, :, 0, j] - g).max() / np.abs(g).max()
        print(f"L * arrivals[{j}] vs {name} dll/d{name}: rel {err:.2e}")
        worst = max(worst, err)
    assert worst < bars.F64_GRADIENT_IDENTITY_BAR, worst


def _kernel16(dbl=False, S=4, L=5000, W=200, seed=5):
    from phlash_amd.kernel import get_kernel

    rows = _rows(S, L, seed=seed, het=0.05, run=300)
    return rows, get_kernel(16, rows, double_precision=dbl, overlap=W)


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_marginals_and_ll_are_phk_posteriors(dbl):
    rows, kern = _kernel16(dbl)
    pp = _bcast(_population(16, 3, seed=2))
    inds = np.arange(4)
    tol = (bars.F64_ARRIVALS_BAR + F64_GAMMA_BAR) if dbl else (bars.F32_ARRIVALS_BAR + F32_GAMMA_BAR)
    for bin in (1, 7):
        t = kern.transitions(pp, inds, bin=bin)
        p = kern.posterior(pp, inds, bin=bin)
        a = t.arrivals.double()
        assert torch.isfinite(a).all() and (a >= 0).all()
        err = float((a.sum(-2) - p.marginals.double()).abs().max())
        print(f"arrivals.sum(-2) vs marginals ({'f64' if dbl else 'f32'}, bin {bin}): max |diff| {err:.2e}")
        assert err < tol
        # changes: the bin sums of the arrivals' up and down rows, reduced over the states
        n = kern.L - kern.overlap
        cnt = torch.as_tensor([min(bin, n - k * bin) for k in range(a.shape[2])], device=a.device, dtype=torch.float64)
        ref = a[..., 1:, :].sum(-1) * cnt[:, None]
        assert float((t.changes.double() - ref).abs().max()) < (1e-12 if dbl else 2e-6) * bin * 4
    for seg, plan in ((0, (0, 4, 8, 4, 0)), (1, (1, 4, 16, 4, 4))):
        kern._eng.set_plan(*plan)
        a = kern.transitions(pp, inds, bin=7, arrivals=False).ll
        b = kern.posterior(pp, inds, bin=7).ll
        assert torch.equal(a, b), (seg, float((a - b).abs().max()))


@pytest.mark.gpu
def test_plans_slabs_and_repeats_are_consistent():
    rows, kern = _kernel16(False)
    eng = kern._eng
    pp = _bcast(_population(16, 3, seed=7))
    inds = np.arange(4)
    lens = np.array([5000, 4321, 5000, 777])
    same = lambda x, y: torch.equal(x.arrivals, y.arrivals) and torch.equal(x.changes, y.changes) and torch.equal(x.ll, y.ll)  # noqa: E731
    ll0, g0 = kern(pp, inds, grad=True)  # the gradient call before any transition call
    plan0 = eng.get_plan()
    a = kern.transitions(pp, inds, bin=7, lens=lens)
    b = kern.transitions(pp, inds, bin=7, lens=lens)
    assert same(a, b)
    ll1, g1 = kern(pp, inds, grad=True)
    assert torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert eng.get_plan() == plan0
    # bins: 7 straddles block, segment and unit edges; 600 is larger than a segment of 512 sites; W = 200 lies inside a block
    # of 16 sites (the segmented plan's)
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        for bin in (7, 600):
            eng.set_plan(*plan)  # (a slab is a launch shape of its own: fix the plan so that both runs use the same one)
            a = kern.transitions(pp, inds, bin=bin, lens=lens)
            eng.set_workspace_limit(1 << 17)  # three sequences per slab
            c = kern.transitions(pp, inds, bin=bin, lens=lens)
            eng.set_workspace_limit(1 << 40)
            assert same(a, c), (plan, bin)
    for bin in (7, 600):
        eng.set_plan(0, 4, 8, 4, 0)
        ser = kern.transitions(pp, inds, bin=bin, lens=lens)
        eng.set_plan(1, 4, 16, 4, 4)
        assert eng.get_plan()["segmented"] == 1
        seg = kern.transitions(pp, inds, bin=bin, lens=lens)
        err = float((ser.arrivals.double() - seg.arrivals.double()).abs().max())
        cs, cg = ser.changes.double(), seg.changes.double()
        errc = float(((cs - cg).abs() / cs.clamp(min=1.0)).max())
        print(f"serial vs segmented plan, bin {bin}: arrivals max |diff| {err:.2e}, changes rel {errc:.2e}")
        assert err < bars.F32_ARRIVALS_BAR and errc < bars.F32_CHANGES_BAR


@pytest.mark.gpu
def test_whole_contigs_padding_counts_nothing():
    import phlash_amd
    from phlash_amd.size_history import DemographicModel

    data, dm, _, _, _ = simulated()
    ws, bin = 100, 10
    dms = [DemographicModel(eta=dm.eta, theta=dm.theta / ws, rho=dm.rho / ws),
           DemographicModel(eta=dm.eta._replace(c=dm.eta.c * 1.5), theta=dm.theta / ws, rho=dm.rho / ws)]
    contigs = [data[:1, :2345], data[1:, :]]  # 2,345 windows end inside a bin of 10 and inside a block
    rag = phlash_amd.posterior_changes(dms[0], contigs, window_size=ws, bin=bin)
    assert [tuple(r.shape) for r in rag] == [(1, 235, 2), (1, 400, 2)] and rag[0].dtype == torch.float64
    for c, r in zip(contigs, rag):
        alone = phlash_amd.posterior_changes(dms[0], c, window_size=ws, bin=bin)
        err = float(((r - alone).abs() / alone.clamp(min=1.0)).max())
        print(f"contig of {c.shape[1]} windows, padded vs alone: rel {err:.2e}")
        assert err < bars.F32_CHANGES_BAR
    both = phlash_amd.posterior_changes(dms, data, window_size=ws, bin=bin)
    each = [phlash_amd.posterior_changes(d, data, window_size=ws, bin=bin) for d in dms]
    assert both.shape == (SIM_ROWS, SIM_SITES // bin, 2) and both.dtype == torch.float64
    assert float((both - (each[0] + each[1]) / 2).abs().max()) < 1e-12 * max(1.0, float(both.abs().max()))


@pytest.mark.gpu
def test_expected_changes_match_the_simulated_path():
    from phlash_amd.kernel import get_kernel

    data, dm, own, exp, se = simulated()
    kern = get_kernel(SIM_K, data, double_precision=False)
    out = kern.transitions(dm, np.arange(SIM_ROWS), bin=1, arrivals=False)
    total = out.changes.double()[:, 1:].sum((1, 2)).cpu().numpy()  # sites 1 .. L-1: z_0 is not part of the simulated path
    print(f"expected TMRCA changes {total} (oracle {exp}), the simulated path's own {own}, standard error {se}")
    assert (np.abs(total - own) < 6 * se).all(), (total, own, se)
    assert (np.abs(total - exp) < bars.F32_CHANGES_BAR * SIM_SITES).all()
