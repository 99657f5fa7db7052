"""Posterior decoding (phk_posterior / HipEngine.posterior / PSMCKernel.posterior / phlash_amd.posterior_tmrca).

CPU: the float64 forward-backward oracle against path enumeration, the ABI's argument check without a device, the lazy
re-export.  GPU: gamma against the oracle for every compiled K (and a padded one) in both precisions, identities that tie
the decode sweep to the shipped gradient call, plans / slabs / repeat calls, one 3,000,001-window row, and recovery of a
simulated coalescence-time path.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import posterior_oracle as po
from oracle import psmc_numpy as pn

# float32 gamma against the float64 oracle, absolute: 5 x the largest error measured on the MI355X over
# test_gamma_against_the_oracle (every K, both parameter layouts, W = 0 / 37, bins 1 / 7 / 100); float64 measured 5.7e-15
F32_GAMMA_BAR = 1.6e-5  # measured worst 3.21e-6 (K = 32)
F64_GAMMA_BAR = 1e-10


def _random_pp(K, rng):
    """a valid SMC' model with K states (random size history), as the oracle's PP"""
    t = np.concatenate([[0.0], np.geomspace(1e-3, 8.0, K - 1)])
    c = np.exp(rng.normal(0, 0.5, K))
    dm = pn.DM(t=t, c=c, theta=0.05 * math.exp(rng.normal()), rho=0.02)
    return pn.from_dm(dm)


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K,L,W", [(2, 6, 0), (3, 6, 2), (4, 5, 0), (4, 5, 3)])
def test_oracle_against_path_enumeration(K, L, W):
    rng = np.random.default_rng(K * 10 + L + W)
    pp = _random_pp(K, rng)
    data = rng.integers(-1, 2, size=L)
    data[0] = 1
    data[L // 2] = -1  # a missing site
    g, ll = po.forward_backward(pp, data, W)
    gb, llb = po.bruteforce(pp, data, W)
    assert g.shape == (L - W, K)
    np.testing.assert_allclose(g, gb, rtol=0, atol=1e-13)
    assert abs(ll - llb) < 1e-12 * abs(llb) + 1e-13
    np.testing.assert_allclose(g.sum(1), 1.0, atol=1e-14)


def test_oracle_ll_is_psmc_ll():
    rng = np.random.default_rng(3)
    pp = _random_pp(8, rng)
    data = (rng.random(300) < 0.05).astype(int)
    data[rng.integers(0, 300, 5)] = -1
    _, ll0 = po.forward_backward(pp, data, 0)
    assert abs(ll0 - pn.psmc_ll(pp, data)[1]) < 1e-12 * abs(ll0)
    _, ll = po.forward_backward(pp, data, 40)
    ref = pn.psmc_ll(pp, data)[1] - pn.psmc_ll(pp, data[:40])[1]
    assert abs(ll - ref) < 1e-11 * abs(ref)


def test_phk_posterior_rejects_a_null_handle_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_posterior" in _lib.SIGNATURES
    rc = lib.phk_posterior(None, None, 0, 0, None, None, 1, 1, 0, 1, None, 0, None, None, None, None)
    assert rc == _lib.PHK_EINVAL
    assert b"NULL" in lib.phk_last_error()


def test_posterior_tmrca_is_lazy_and_has_no_cpu_fallback(monkeypatch):
    import phlash_amd

    f = phlash_amd.posterior_tmrca
    from phlash_amd.decode import posterior_tmrca

    assert f is posterior_tmrca
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dm = phlash_amd.DemographicModel.default("4*1", 1e-4, 1e-4)
    data = np.zeros((1, 50), dtype=np.int8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        posterior_tmrca(dm, data)


# ------------------------------------------------------------------------------------------------- GPU helpers
def _population(K, B, seed):
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population

    tmpl, x = particle_population(K, B, seed=seed, sigma=0.25)
    return PSMCParams.from_dm(tmpl.from_flat(x).to_dm())  # fields [B, K] float64


def _rows(S, L, seed, het=0.03, miss=0.01, run=None):
    rng = np.random.default_rng(seed)
    d = (rng.random((S, L)) < het).astype(np.int8)
    d.flat[rng.integers(0, d.size, int(miss * d.size))] = -1
    if run is not None:  # runs of missing windows (an accessibility mask): the *_mr forward kernels
        for s in range(S):
            a = rng.integers(0, L - run)
            d[s, a : a + run] = -1
    d[:, 0] = 1
    return d


def _pp_np(pp, b):
    return pn.PP(*(np.asarray(getattr(pp, f)[b].cpu().numpy() if isinstance(getattr(pp, f), torch.Tensor) else getattr(pp, f)[b],
                              float) for f in pn.PP._fields))


def _oracle(pp, data, W, bin, values, per_chunk=False):
    """-> marginals [B, S, nbin, K], mean [B, S, nbin], ll [B, S] for per-particle blocks broadcast over the rows, fields
    [B, K]; ``per_chunk``: for one block per (particle, chunk), fields [B * S, K]"""
    S = len(data)
    B = pp.d.shape[0] // (S if per_chunk else 1)
    M, MU, LL = [], [], []
    for b in range(B):
        ms, mus, lls = [], [], []
        for s, row in enumerate(data):
            q = _pp_np(pp, b * S + s if per_chunk else b)
            g, ll = po.forward_backward(q, row, W)
            ms.append(po.bin_means(g, bin))
            mus.append(po.bin_means(g @ values[b], bin))
            lls.append(ll)
        M.append(ms)
        MU.append(mus)
        LL.append(lls)
    return np.array(M), np.array(MU), np.array(LL)


def _bcast(pp):
    from phlash_amd.params import PSMCParams

    return PSMCParams(*(torch.as_tensor(a)[:, None] for a in pp))


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
@pytest.mark.parametrize("K", [4, 8, 12, 16, 32, 64])
def test_gamma_against_the_oracle(K, dbl):
    from phlash_amd.kernel import get_kernel

    B, S, L = 2, 3, 700
    pp = _population(K, B, seed=K)
    pc = _population(K, B * S, seed=1000 + K)  # the "chunk" layout: one model per (particle, chunk), all different
    values = np.stack([np.linspace(0.1, 5.0, K), np.arange(K, dtype=float)])
    worst = 0.0
    for rows, W in ((_rows(S, L, seed=1), 0), (_rows(S, L, seed=2, run=120), 37)):
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        for bin in (1, 7, 100):
            for layout in ("bcast", "chunk"):
                if layout == "bcast":
                    q = _bcast(pp)
                    M, MU, LL = _oracle(pp, rows, W, bin, values)
                else:  # one block per (particle, chunk), compared per chunk
                    from phlash_amd.params import PSMCParams

                    q = PSMCParams(*(torch.as_tensor(a).reshape(B, S, K).contiguous() for a in pc))
                    M, MU, LL = _oracle(pc, rows, W, bin, values, per_chunk=True)
                out = kern.posterior(q, np.arange(S), values=values, bin=bin)
                m = out.marginals.double().cpu().numpy()
                mu = out.mean.double().cpu().numpy()
                assert m.shape == M.shape and mu.shape == MU.shape
                err = max(np.abs(m - M).max(), np.abs(mu - MU).max() / np.abs(values).max())
                worst = max(worst, err)
                rel = np.abs(out.ll.cpu().numpy() / LL - 1).max()
                assert rel < (1e-12 if dbl else 1e-5), (bin, layout, W, rel)
    print(f"PARITY posterior K={K} {'f64' if dbl else 'f32'}: max |gamma - oracle| = {worst:.3e}")
    assert worst < (F64_GAMMA_BAR if dbl else F32_GAMMA_BAR), worst


def _kernel16(dbl=False, S=4, L=5000, W=200, seed=5):
    from phlash_amd.kernel import get_kernel

    rows = _rows(S, L, seed=seed, het=0.05, run=300)
    return rows, get_kernel(16, rows, double_precision=dbl, overlap=W)


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_identities(dbl):
    rows, kern = _kernel16(dbl)
    pp = _bcast(_population(16, 3, seed=2))
    f = np.linspace(0.0, 3.0, 16)
    one = kern.posterior(pp, np.arange(4), values=f, bin=1)
    tol = 1e-12 if dbl else 2e-6
    m1 = one.marginals.double()
    assert torch.isfinite(m1).all() and (m1 >= 0).all()
    assert float((m1.sum(-1) - 1).abs().max()) < tol * 16
    ft = torch.as_tensor(f, device=m1.device)
    assert float((one.mean.double() - m1 @ ft).abs().max()) < tol * 16 * 3
    for bin in (7, 100):
        out = kern.posterior(pp, np.arange(4), values=f, bin=bin)
        n = m1.shape[2]
        nb = (n + bin - 1) // bin
        ref = torch.stack([m1[:, :, k * bin : min((k + 1) * bin, n)].mean(2) for k in range(nb)], 2)
        assert float((out.marginals.double() - ref).abs().max()) < tol * 8
        assert torch.equal(out.ll, one.ll)
    # ll: the forward leg's by-product, against a no-gradient loglik on a forced plan (same forward variant)
    for seg in (0, 1):
        kern._eng.set_plan(seg, 4, 8, 4, 4)
        a = kern.posterior(pp, np.arange(4), values=f).ll
        b = kern.loglik(pp, np.arange(4))
        rel = float((a / b - 1).abs().max())
        print(f"posterior ll vs no-gradient loglik ({'f64' if dbl else 'f32'}, plan segmented={seg}): "
              f"rel {rel:.2e}, bitwise {bool(torch.equal(a, b))}")
        assert rel <= 1e-12


@pytest.mark.gpu
def test_het_mass_matches_the_gradient_call():
    """At W = 0, sum over het sites of gamma_t(k) = e1_k d ll / d e1_k: the posterior mass the shipped gradient sweep books."""
    from phlash_amd.kernel import get_kernel

    rows = _rows(3, 3000, seed=11, het=0.04)
    kern = get_kernel(16, rows, double_precision=True, overlap=0)
    pp = _population(16, 2, seed=4)
    q = _bcast(pp)
    g = kern.posterior(q, np.arange(3), bin=1).marginals.double().cpu().numpy()  # [B, S, L, K]
    het = (rows == 1)[None, :, :, None]
    mass = (g * het).sum(2)
    _, dll = kern(q, np.arange(3), grad=True)
    e1 = np.asarray(dll.emis1.cpu().numpy() if isinstance(dll.emis1, torch.Tensor) else dll.emis1)
    err = np.abs(mass - e1).max() / np.abs(e1).max()
    print(f"het mass vs e1 dll/de1: rel {err:.2e}")
    assert err < 1e-9


@pytest.mark.gpu
def test_plans_slabs_and_repeats_are_consistent():
    rows, kern = _kernel16(False)
    eng = kern._eng
    pp = _bcast(_population(16, 3, seed=7))
    inds = np.arange(4)
    f = np.linspace(0.0, 3.0, 16)
    ll0, g0 = kern(pp, inds, grad=True)  # the gradient call before any decode
    plan0 = eng.get_plan()
    a = kern.posterior(pp, inds, values=f, bin=7)
    b = kern.posterior(pp, inds, values=f, bin=7)
    assert torch.equal(a.marginals, b.marginals) and torch.equal(a.mean, b.mean) and torch.equal(a.ll, b.ll)
    ll1, g1 = kern(pp, inds, grad=True)
    assert torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert eng.get_plan() == plan0
    eng.set_plan(0, 4, 8, 4, 0)  # (a slab is a launch shape of its own: fix the plan so that both runs use the same one)
    a = kern.posterior(pp, inds, values=f, bin=7)
    eng.set_workspace_limit(1 << 17)  # three sequences per slab
    c = kern.posterior(pp, inds, values=f, bin=7)
    assert torch.equal(a.marginals, c.marginals) and torch.equal(a.mean, c.mean) and torch.equal(a.ll, c.ll)
    eng.set_workspace_limit(1 << 40)
    eng.set_plan(0, 4, 8, 4, 0)
    ser = kern.posterior(pp, inds, values=f, bin=7)
    eng.set_plan(1, 4, 16, 4, 4)
    seg = kern.posterior(pp, inds, values=f, bin=7)
    err = float((ser.marginals.double() - seg.marginals.double()).abs().max())
    print(f"serial vs segmented plan: max |diff| {err:.2e}")
    assert err < F32_GAMMA_BAR


@pytest.mark.gpu
def test_one_row_of_3_000_001_windows_segmented():
    from phlash_amd.engine import HipEngine

    L = 3_000_001
    rng = np.random.default_rng(9)
    data = (rng.random((1, L), dtype=np.float32) < 0.05).astype(np.int8)
    data.flat[rng.integers(0, L, L // 100)] = -1
    data[0, 0] = 1
    eng = HipEngine(16, data, double_precision=False)
    eng.set_plan(1, 4, 8, 16, 16)  # segmented: the one-state-per-lane forward kernel and beta scan, decode units
    P = _population(16, 1, seed=3)
    P = torch.stack(list(P), -2)[:, None].cuda()
    inds = torch.zeros(1, dtype=torch.int64, device="cuda")
    f = torch.linspace(0.0, 3.0, 16, dtype=torch.float64, device="cuda")
    ll, mean, marg = eng.posterior(P, inds, 1, values=f, bin=1, marginals=True, mean=True)
    assert not eng.underflow_risk()
    assert torch.isfinite(marg).all() and torch.isfinite(mean).all()
    assert marg.shape == (1, 1, L - 1, 16)
    assert float((marg.double().sum(-1) - 1).abs().max()) < 3e-5
    assert float((mean.double() - marg.double() @ f).abs().max()) < 1e-4
    ll_ref = eng.run(P, inds, 1, grad=False)
    rel = float((ll / ll_ref - 1).abs().max())
    print(f"3,000,001-window row: ll rel to the no-gradient call {rel:.2e}, bitwise {bool(torch.equal(ll, ll_ref))}")
    assert rel <= 1e-12
    _, _, m100 = eng.posterior(P, inds, 1, bin=100)
    ref = marg[0, 0, : (L - 1) // 100 * 100].double().reshape(-1, 100, 16).mean(1)
    assert float((m100[0, 0, : ref.shape[0]].double() - ref).abs().max()) < 1e-5


def simulate_with_path(K, n_rows, n_sites, seed, theta=1e-2, rho=1e-2, missing=0.01):
    """synth.simulate_chunks' recipe, also returning the hidden path z [n_rows, n_sites] (the state after each site's
    transition) and the model it was drawn from"""
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel
    from phlash_amd.transition import transition_matrix

    rng = np.random.default_rng(seed)
    dm = DemographicModel.default(f"{K}*1", theta, rho)
    A = np.clip(transition_matrix(dm).numpy(), 0.0, None)
    cumA = np.cumsum(A / A.sum(1, keepdims=True), axis=1)
    pp = PSMCParams.from_dm(dm)
    emis1 = pp.emis1.numpy()
    cum_pi = np.cumsum(pp.pi.numpy() / pp.pi.numpy().sum())
    z = np.minimum((rng.uniform(size=n_rows)[:, None] > cum_pi[None]).sum(1), K - 1)
    out = np.empty((n_rows, n_sites), dtype=np.int8)
    path = np.empty((n_rows, n_sites), dtype=np.int64)
    for t in range(n_sites):
        z = np.minimum((rng.uniform(size=n_rows)[:, None] > cumA[z]).sum(1), K - 1)
        path[:, t] = z
        out[:, t] = rng.uniform(size=n_rows) < emis1[z]
    out.flat[rng.integers(0, out.size, size=int(missing * out.size))] = -1
    out[:, 0] = np.maximum(out[:, 0], 0)
    return out, path, dm


# correlation of the posterior mean state with the true state, 4 rows x 50,000 windows at theta = rho = 0.05 per window:
# 0.715 measured on the MI355X (the smallest of the four rows); the bar leaves a margin
RECOVERY_MIN_CORR = 0.6


@pytest.mark.gpu
def test_recovers_the_simulated_path_and_averages_models():
    import phlash_amd
    from phlash_amd.size_history import DemographicModel

    K = 16
    data, path, dm = simulate_with_path(K, 4, 50_000, seed=21, theta=0.05, rho=0.05)
    from phlash_amd.kernel import get_kernel

    kern = get_kernel(K, data, double_precision=False)
    out = kern.posterior(dm, np.arange(4), values=np.arange(K, dtype=float), bin=1, marginals=False)
    est = out.mean.double().cpu().numpy()
    corr = min(np.corrcoef(est[s], path[s])[0, 1] for s in range(4))
    print(f"posterior mean state vs true state: min correlation over rows {corr:.3f}")
    assert corr > RECOVERY_MIN_CORR
    # posterior_tmrca: per base pair rates, averaged over models with equal weight
    ws = 100
    dms = [DemographicModel(eta=dm.eta, theta=dm.theta / ws, rho=dm.rho / ws),
           DemographicModel(eta=dm.eta._replace(c=dm.eta.c * 1.5), theta=dm.theta / ws, rho=dm.rho / ws)]
    both = phlash_amd.posterior_tmrca(dms, data, window_size=ws, bin=10)
    each = [phlash_amd.posterior_tmrca(d, data, window_size=ws, bin=10) for d in dms]
    assert both.shape == (4, 5000) and both.dtype == torch.float64
    assert float((both - (each[0] + each[1]) / 2).abs().max()) < 1e-5 * float(both.abs().max())
    # ragged contigs: padded with missing windows, stripped again; a missing tail changes the real sites by rounding only
    from phlash_amd.data import RawContig

    cs = [RawContig(data[:2, :30_000], np.ones(1), ws), RawContig(data[2:, :], np.ones(1), ws)]
    rag = phlash_amd.posterior_tmrca(dms[0], cs, window_size=ws, bin=10)
    assert [r.shape for r in rag] == [(2, 3000), (2, 5000)]
    alone = phlash_amd.posterior_tmrca(dms[0], data[:2, :30_000], window_size=ws, bin=10)
    err = float((rag[0] - alone).abs().max() / alone.abs().max())
    print(f"padded vs unpadded contig: rel {err:.2e}")
    assert err < 1e-4
    assert float((rag[1] - each[0][2:]).abs().max() / each[0].abs().max()) < 1e-5
