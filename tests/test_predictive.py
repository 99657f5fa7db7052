"""Leave-one-out predictive decoding (phk_predictive / HipEngine.predictive / PSMCKernel.predictive / phlash_amd.predictive_check).

CPU: the float64 dense oracle against path enumeration, against the likelihood-ratio identity through the forward-backward
oracle's ll, and against the gamma identity at missing sites; the structured (loop-form) statement of the kernel's arithmetic
against the dense oracle on the GPU grid's inputs; the ABI's argument check without a device; the lazy re-export; and the
simulated rows' own het count against the oracle's expectation.
GPU: the track against the oracle for every compiled K (and a padded one) in both precisions with ragged lens, the
likelihood-ratio identity against the shipped no-gradient call, the missing-site identity against phk_posterior, ll bitwise
phk_posterior's, plans / slabs / repeat calls, whole contigs of different lengths, and the calibration on simulated rows.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import posterior_oracle as po
import predictive_bars as bars
import predictive_oracle as lo
from test_posterior_decode import F32_GAMMA_BAR, F64_GAMMA_BAR, _bcast, _pp_np, _population, _random_pp, _rows, simulate_with_path

GRID_K = [4, 8, 12, 16, 32, 64]
GRID_B, GRID_S, GRID_L = 2, 3, 700
GRID_BINS = (1, 7, 100)


# ------------------------------------------------------------------------------------------------- shared inputs
def grid_sets():
    """The two row sets of the oracle grid: (rows, W, lens), those of the transition-posterior grid.  Rows with isolated missing
    sites (both) and with runs of 120 missing windows (the second).  lens: 593 and 437 end inside a block (of 8 and of 16 sites)
    and inside a bin of 7; 300 (W = 0) and 437 (W = 37) leave whole bins of 100 without a site of the row's own; 655 ends inside
    a bin of 100.  The first set keeps its data past the own lengths (the mask alone), row 0 of the second is padded with missing
    windows past its own length."""
    r1 = _rows(GRID_S, GRID_L, seed=1)
    r2 = _rows(GRID_S, GRID_L, seed=2, run=120)
    r2[0, 437:] = -1
    return [(r1, 0, np.array([700, 593, 300])), (r2, 37, np.array([437, 700, 655]))]


@functools.lru_cache(maxsize=None)
def grid_oracle(K):
    """-> {(set, layout): (phet [B, S, L - W], score [B, S, L - W], ll [B, S])} of the dense float64 oracle, once per K"""
    pp = _population(K, GRID_B, seed=K)
    pc = _population(K, GRID_B * GRID_S, seed=1000 + K)  # one model per (particle, chunk), all different
    out = {}
    for i, (rows, W, _) in enumerate(grid_sets()):
        for layout in ("bcast", "chunk"):
            ph = np.empty((GRID_B, GRID_S, GRID_L - W))
            sc = np.empty((GRID_B, GRID_S, GRID_L - W))
            ll = np.empty((GRID_B, GRID_S))
            for b in range(GRID_B):
                for s in range(GRID_S):
                    q = _pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * GRID_S + s)
                    ph[b, s], sc[b, s], ll[b, s] = lo.loo(q, rows[s], W)
            ph.setflags(write=False)
            sc.setflags(write=False)
            out[i, layout] = (ph, sc, ll)
    return out


def _binned(ph, sc, rows, W, bin, lens):
    """per-site oracle [B, S, n] -> track [B, S, nbin, 3]"""
    return np.array([[lo.reduce_bins(ph[b, s], sc[b, s], rows[s], W, bin, None if lens is None else int(lens[s]))
                      for s in range(ph.shape[1])] for b in range(ph.shape[0])])


def _errors(t, T):
    """(largest absolute error of the het entries, largest error of the score entry relative to max(1, |oracle|))"""
    return np.abs(t[..., :2] - T[..., :2]).max(), (np.abs(t[..., 2] - T[..., 2]) / np.maximum(1.0, np.abs(T[..., 2]))).max()


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K,L,W", [(2, 6, 0), (3, 6, 2), (4, 5, 0), (4, 5, 3)])
def test_oracle_against_path_enumeration(K, L, W):
    rng = np.random.default_rng(K * 10 + L + W)
    pp = _random_pp(K, rng)
    data = rng.integers(-1, 2, size=L)
    data[0] = 1  # a het at site 0
    data[L // 2] = -1  # a missing site mid-row
    ph, sc, ll = lo.loo(pp, data, W)
    pb, sb = lo.bruteforce_loo(pp, data, W)
    assert ph.shape == (L - W,) and sc.shape == (L - W,)
    np.testing.assert_allclose(ph, pb, rtol=0, atol=1e-13)
    np.testing.assert_allclose(sc, sb, rtol=0, atol=1e-13)
    assert (sc <= 0).all() and (sc[data[W:] < 0] == 0).all()
    _, llb = po.bruteforce(pp, data, W)
    assert abs(ll - llb) < 1e-12 * abs(llb) + 1e-13
    # the masked, binned reduction by hand
    length = L - 1
    T = lo.reduce_bins(ph, sc, data, W, 2, length)
    n_own = length - W
    obs = data[W:] >= 0
    assert T.shape == ((L - W + 1) // 2, 3)
    assert abs(T[:, 0].sum() - ph[:n_own][obs[:n_own]].sum()) < 1e-14
    assert abs(T[:, 1].sum() - ph[:n_own][~obs[:n_own]].sum()) < 1e-14
    assert abs(T[:, 2].sum() - sc[:n_own].sum()) < 1e-14
    assert not T[(n_own - 1) // 2 + 1 :].any()


def test_oracle_against_the_likelihood_ratio():
    """phet_t = 1 / (1 + exp(ll(o with o_t := hom) - ll(o with o_t := het))) through forward_backward's ll"""
    rng = np.random.default_rng(5)
    K, L, W = 8, 60, 7
    pp = _random_pp(K, rng)
    data = (rng.random(L) < 0.1).astype(int)
    data[rng.integers(0, L, 3)] = -1
    data[30:36] = -1
    ph, sc, ll = lo.loo(pp, data, W)
    _, llg = po.forward_backward(pp, data, W)
    assert abs(ll - llg) < 1e-12 * abs(llg)
    worst = 0.0
    for t in range(W, L):
        d0, d1 = data.copy(), data.copy()
        d0[t], d1[t] = 0, 1
        l0, l1 = po.forward_backward(pp, d0, W)[1], po.forward_backward(pp, d1, W)[1]
        ref = 1.0 / (1.0 + np.exp(l0 - l1))
        worst = max(worst, abs(ph[t - W] - ref))
        if data[t] >= 0:
            worst = max(worst, abs(sc[t - W] - np.log(ref if data[t] >= 1 else 1.0 - ref)))
    print(f"oracle vs likelihood ratio: max |diff| = {worst:.3e}")
    assert worst < 1e-12


def test_oracle_against_gamma_at_missing_sites():
    """at a missing site the cavity weight IS the posterior: phet_t = sum_k gamma_t(k) emis1(k) / sum_k gamma_t(k) (emis0 + emis1)(k)"""
    rng = np.random.default_rng(6)
    for K, W in ((4, 0), (8, 0), (16, 40)):
        pp = _random_pp(K, rng)
        data = (rng.random(300) < 0.05).astype(int)
        data[rng.integers(0, 300, 5)] = -1
        data[100:130] = -1
        ph, sc, _ = lo.loo(pp, data, W)
        g, _ = po.forward_backward(pp, data, W)
        e0, e1 = np.asarray(pp.emis0, float), np.asarray(pp.emis1, float)
        miss = data[W:] < 0
        assert miss.sum() >= 30
        ref = (g @ e1) / (g @ (e0 + e1))
        assert np.abs(ph[miss] - ref[miss]).max() < 1e-13
        assert (sc[miss] == 0).all()


@functools.lru_cache(maxsize=None)
def structured_floor(K):
    """the structured float64 statement against the dense oracle on the GPU grid's inputs (every particle and row of both sets
    in both parameter layouts), in the GPU grid's own metric: binned with the grid's bins and lens -> (het, score) errors"""
    pp = _population(K, GRID_B, seed=K)
    pc = _population(K, GRID_B * GRID_S, seed=1000 + K)
    worst_h = worst_s = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        for layout in ("bcast", "chunk"):
            ph, sc, _ = grid_oracle(K)[i, layout]
            for b in range(GRID_B):
                for s in range(GRID_S):
                    p, c = lo.structured(_pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * GRID_S + s), rows[s], W)
                    for bin in GRID_BINS:
                        eh, es = _errors(lo.reduce_bins(p, c, rows[s], W, bin, int(lens[s])),
                                         lo.reduce_bins(ph[b, s], sc[b, s], rows[s], W, bin, int(lens[s])))
                        worst_h, worst_s = max(worst_h, eh), max(worst_s, es)
    return worst_h, worst_s


@pytest.mark.parametrize("K", GRID_K)
def test_structured_statement_against_the_dense_oracle(K):
    """The kernel's form in float64 loops (folded factors, exclusive prefix / suffix, table rows, per-site ratio) against the
    dense oracle: the float64 rounding floor the GPU bars are judged against (predictive_bars.STRUCTURED_*_FLOOR)."""
    worst_h, worst_s = structured_floor(K)
    print(f"PARITY predictive structured-vs-dense K={K}: max |het - oracle| = {worst_h:.3e}, max |score - oracle| / max(1, |oracle|) = {worst_s:.3e}")
    assert worst_h < bars.STRUCTURED_HET_FLOOR_BAR and worst_s < bars.STRUCTURED_SCORE_FLOOR_BAR, (worst_h, worst_s)


def test_float64_bars_are_within_ten_floors():
    assert bars.F64_HET_BAR <= 10 * bars.STRUCTURED_HET_FLOOR
    assert bars.F64_SCORE_BAR <= 10 * bars.STRUCTURED_SCORE_FLOOR


def test_phk_predictive_rejects_a_null_handle_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_predictive" in _lib.SIGNATURES
    rc = lib.phk_predictive(None, None, 0, 0, None, None, 1, 1, 0, 1, None, None, None, None)
    assert rc == _lib.PHK_EINVAL
    assert b"NULL" in lib.phk_last_error()


def test_predictive_check_is_lazy_and_has_no_cpu_fallback(monkeypatch):
    import phlash_amd

    f = phlash_amd.predictive_check
    from phlash_amd.decode import predictive_check

    assert f is predictive_check
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dm = phlash_amd.DemographicModel.default("4*1", 1e-4, 1e-4)
    data = np.zeros((1, 50), dtype=np.int8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        predictive_check(dm, data)


SIM_K, SIM_ROWS, SIM_SITES, SIM_SEED = 16, 2, 4000, 21


@functools.lru_cache(maxsize=None)
def simulated():
    """-> (data, dm, the rows' own het counts, the oracle's sum of phet over the observed sites, its standard error from the
    per-site het probabilities treated as independent)"""
    from phlash_amd.params import PSMCParams

    data, _, dm = simulate_with_path(SIM_K, SIM_ROWS, SIM_SITES, seed=SIM_SEED, theta=0.05, rho=0.05)
    pp = PSMCParams.from_dm(dm)
    q = _pp_np(PSMCParams(*(torch.as_tensor(a)[None] for a in pp)), 0)
    own = (data >= 1).sum(1)
    exp, se = np.empty(SIM_ROWS), np.empty(SIM_ROWS)
    for s in range(SIM_ROWS):
        ph, _, _ = lo.loo(q, data[s], 0)
        p = ph[data[s] >= 0]
        exp[s], se[s] = p.sum(), np.sqrt((p * (1 - p)).sum())
    return data, dm, own, exp, se


def test_simulated_seed_lies_inside_the_bar():
    _, _, own, exp, se = simulated()
    print(f"simulated rows: own het windows {own}, oracle's expectation {exp}, standard error {se}")
    assert (own > 50).all()
    assert (np.abs(own - exp) < 6 * se).all(), (own, exp, se)


# ------------------------------------------------------------------------------------------------- GPU
def _track(out):
    return torch.stack([out.het_observed, out.het_missing, out.score], -1).double().cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
@pytest.mark.parametrize("K", GRID_K)
def test_predictive_against_the_oracle(K, dbl):
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    B, S = GRID_B, GRID_S
    pp = _population(K, B, seed=K)
    pc = _population(K, B * S, seed=1000 + K)
    worst_h = worst_s = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        for layout in ("bcast", "chunk"):
            ph, sc, LL = grid_oracle(K)[i, layout]
            q = _bcast(pp) if layout == "bcast" else PSMCParams(*(torch.as_tensor(a).reshape(B, S, K).contiguous() for a in pc))
            for bin in GRID_BINS:
                T = _binned(ph, sc, rows, W, bin, lens)
                out = kern.predictive(q, np.arange(S), bin=bin, lens=lens)
                t = _track(out)
                assert t.shape == T.shape
                assert np.isfinite(t).all()
                eh, es = _errors(t, T)
                worst_h, worst_s = max(worst_h, eh), max(worst_s, es)
                # a bin without a site of the row's own is zeros, exactly
                n = GRID_L - W
                empty = np.array([[min((k + 1) * bin, n, int(lens[s]) - W) <= k * bin for k in range(T.shape[2])] for s in range(S)])
                assert empty.any()
                assert not t[:, empty].any() and not T[:, empty].any()
                rel = np.abs(out.ll.cpu().numpy() / LL - 1).max()
                assert rel < (1e-12 if dbl else 1e-5), (bin, layout, W, rel)
    print(f"PARITY predictive K={K} {'f64' if dbl else 'f32'}: max |het - oracle| = {worst_h:.3e}, "
          f"max |score - oracle| / max(1, |oracle|) = {worst_s:.3e}")
    assert worst_h < (bars.F64_HET_BAR if dbl else bars.F32_HET_BAR), worst_h
    assert worst_s < (bars.F64_SCORE_BAR if dbl else bars.F32_SCORE_BAR), worst_s
    if dbl:
        assert bars.F64_HET_BAR <= 10 * bars.STRUCTURED_HET_FLOOR and bars.F64_SCORE_BAR <= 10 * bars.STRUCTURED_SCORE_FLOOR


@pytest.mark.gpu
def test_likelihood_ratio_identity_against_loglik():
    """phet_t = 1 / (1 + exp(ll(o with o_t := hom) - ll(o with o_t := het))) with both ll from the shipped no-gradient call: code
    that shares only the forward step with the predictive sweep."""
    from phlash_amd.kernel import get_kernel

    L = 200
    rng = np.random.default_rng(17)
    base = (rng.random(L) < 0.05).astype(np.int8)
    base[90:100] = -1  # a missing run
    base[150] = -1  # an isolated missing site
    base[39:42] = (0, 1, 0)  # a het site
    base[0] = 1
    probes = [0, 7, 8, 15, 16, 95, 199, 150, 40]
    assert base[95] == -1 and base[149] >= 0 and base[151] >= 0 and base[40] == 1
    rows = [base]
    for t in probes:
        for o in (0, 1):
            r = base.copy()
            r[t] = o
            rows.append(r)
    data = np.stack(rows)
    kern = get_kernel(16, data, double_precision=True, overlap=0)
    q = _population(16, 2, seed=4)
    out = kern.predictive(_bcast(q), np.arange(1), bin=1)
    ph = (out.het_observed + out.het_missing).double().cpu().numpy()[:, 0]  # [B, L]: one of the two is exactly 0 at every site
    ll = kern(_bcast(q), np.arange(data.shape[0]), grad=False)
    ll = np.asarray(ll.cpu().numpy() if isinstance(ll, torch.Tensor) else ll, float)  # [B, 1 + 2 * probes]
    worst = 0.0
    for j, t in enumerate(probes):
        ref = 1.0 / (1.0 + np.exp(ll[:, 1 + 2 * j] - ll[:, 2 + 2 * j]))
        err = np.abs(ph[:, t] - ref).max()
        print(f"site {t} (o = {base[t]}): phet {ph[:, t]}, likelihood ratio {ref}, |diff| {err:.2e}")
        worst = max(worst, err)
    print(f"PARITY predictive likelihood-ratio identity: max |diff| = {worst:.3e}")
    assert bars.F64_LIKELIHOOD_RATIO_BAR < 1e-10
    assert worst < bars.F64_LIKELIHOOD_RATIO_BAR, worst


def _kernel16(dbl=False, S=4, L=5000, W=200, seed=5):
    from phlash_amd.kernel import get_kernel

    rows = _rows(S, L, seed=seed, het=0.05, run=300)
    return rows, get_kernel(16, rows, double_precision=dbl, overlap=W)


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_missing_sites_are_phk_posteriors(dbl):
    rows, kern = _kernel16(dbl)
    q = _population(16, 3, seed=2)
    pp = _bcast(q)
    inds = np.arange(4)
    tol = (bars.F64_HET_BAR + F64_GAMMA_BAR) if dbl else (bars.F32_HET_BAR + F32_GAMMA_BAR)
    out = kern.predictive(pp, inds, bin=1)
    g = kern.posterior(pp, inds, bin=1).marginals.double()  # [B, S, n, K]
    e0 = torch.as_tensor(np.asarray(q.emis0), dtype=torch.float64, device=g.device)[:, None, None, :]
    e1 = torch.as_tensor(np.asarray(q.emis1), dtype=torch.float64, device=g.device)[:, None, None, :]
    ref = (g * e1).sum(-1) / (g * (e0 + e1)).sum(-1)
    miss = torch.as_tensor(rows[:, kern.overlap :] < 0, device=g.device)[None].expand(3, -1, -1)
    assert int(miss.sum()) > 3 * 4 * 300
    ho, hm, sc = out.het_observed.double(), out.het_missing.double(), out.score.double()
    assert torch.isfinite(ho).all() and torch.isfinite(hm).all() and torch.isfinite(sc).all()
    err = float((hm - ref)[miss].abs().max())
    print(f"het_missing vs marginals ({'f64' if dbl else 'f32'}): max |diff| {err:.2e}")
    assert err < tol
    assert not ho[miss].any() and not hm[~miss].any()
    assert (ho[~miss] > 0).all() and (hm[miss] > 0).all()
    assert (sc <= 0).all() and not sc[miss].any()


@pytest.mark.gpu
def test_ll_is_bitwise_phk_posteriors():
    rows, kern = _kernel16(False)
    pp = _bcast(_population(16, 3, seed=2))
    inds = np.arange(4)
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        kern._eng.set_plan(*plan)
        a = kern.predictive(pp, inds, bin=7).ll
        b = kern.posterior(pp, inds, bin=7).ll
        assert torch.equal(a, b), (plan, float((a - b).abs().max()))


@pytest.mark.gpu
def test_plans_slabs_and_repeats_are_consistent():
    rows, kern = _kernel16(False)
    eng = kern._eng
    pp = _bcast(_population(16, 3, seed=7))
    inds = np.arange(4)
    lens = np.array([5000, 4321, 5000, 777])
    same = lambda x, y: all(torch.equal(p, q) for p, q in zip(x, y))  # noqa: E731
    ll0, g0 = kern(pp, inds, grad=True)  # the gradient call before any predictive call
    plan0 = eng.get_plan()
    a = kern.predictive(pp, inds, bin=7, lens=lens)
    b = kern.predictive(pp, inds, bin=7, lens=lens)
    assert same(a, b)
    ll1, g1 = kern(pp, inds, grad=True)
    assert torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert eng.get_plan() == plan0
    # bins: 7 straddles block, segment and unit edges; 600 is larger than a segment of 512 sites; W = 200 lies inside a block
    # of 16 sites (the segmented plan's)
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        for bin in (7, 600):
            eng.set_plan(*plan)  # (a slab is a launch shape of its own: fix the plan so that both runs use the same one)
            a = kern.predictive(pp, inds, bin=bin, lens=lens)
            eng.set_workspace_limit(1 << 17)  # three sequences per slab
            c = kern.predictive(pp, inds, bin=bin, lens=lens)
            eng.set_workspace_limit(1 << 40)
            assert same(a, c), (plan, bin)
    for bin in (7, 600):
        eng.set_plan(0, 4, 8, 4, 0)
        ser = _track(kern.predictive(pp, inds, bin=bin, lens=lens))
        eng.set_plan(1, 4, 16, 4, 4)
        assert eng.get_plan()["segmented"] == 1
        seg = _track(kern.predictive(pp, inds, bin=bin, lens=lens))
        eh, es = _errors(seg, ser)
        print(f"serial vs segmented plan, bin {bin}: het max |diff| {eh:.2e}, score rel {es:.2e}")
        assert eh < bars.F32_HET_BAR and es < bars.F32_SCORE_BAR


@pytest.mark.gpu
def test_whole_contigs_padding_counts_nothing():
    import phlash_amd
    from phlash_amd.size_history import DemographicModel

    data, dm, _, _, _ = simulated()
    ws, bin = 100, 10
    dms = [DemographicModel(eta=dm.eta, theta=dm.theta / ws, rho=dm.rho / ws),
           DemographicModel(eta=dm.eta._replace(c=dm.eta.c * 1.5), theta=dm.theta / ws, rho=dm.rho / ws)]
    contigs = [data[:1, :2345], data[1:, :]]  # 2,345 windows end inside a bin of 10 and inside a block
    rag = phlash_amd.predictive_check(dms[0], contigs, window_size=ws, bin=bin)
    assert [tuple(r.shape) for r in rag] == [(1, 235, 5), (1, 400, 5)] and rag[0].dtype == torch.float64
    for c, r in zip(contigs, rag):
        alone = phlash_amd.predictive_check(dms[0], c, window_size=ws, bin=bin)
        r, alone = r.cpu().numpy(), alone.cpu().numpy()
        eh, es = _errors(r, alone)
        print(f"contig of {c.shape[1]} windows, padded vs alone: het max |diff| {eh:.2e}, score rel {es:.2e}")
        assert eh < bars.F32_HET_BAR and es < bars.F32_SCORE_BAR
        assert np.array_equal(r[..., 3:], alone[..., 3:])
        # the data's own columns against a numpy count
        n = c.shape[1]
        for k in range(r.shape[1]):
            w = c[0, k * bin : min((k + 1) * bin, n)]
            assert r[0, k, 3] == (w >= 1).sum() and r[0, k, 4] == (w >= 0).sum()
    both = phlash_amd.predictive_check(dms, data, window_size=ws, bin=bin)
    each = [phlash_amd.predictive_check(d, data, window_size=ws, bin=bin) for d in dms]
    assert both.shape == (SIM_ROWS, SIM_SITES // bin, 5) and both.dtype == torch.float64
    assert float((both - (each[0] + each[1]) / 2).abs().max()) < 1e-12 * max(1.0, float(both.abs().max()))
    assert float(both[..., 3].sum()) == (data >= 1).sum() and float(both[..., 4].sum()) == (data >= 0).sum()


@pytest.mark.gpu
def test_expected_hets_match_the_simulated_rows():
    from phlash_amd.kernel import get_kernel

    data, dm, own, exp, se = simulated()
    kern = get_kernel(SIM_K, data, double_precision=False)
    out = kern.predictive(dm, np.arange(SIM_ROWS), bin=1)
    total = out.het_observed.double().sum(-1).cpu().numpy()
    print(f"expected het windows {total} (oracle {exp}), the rows' own {own}, standard error {se}")
    assert (np.abs(total - own) < 6 * se).all(), (total, own, se)
    assert (np.abs(total - exp) < bars.F32_HET_BAR * SIM_SITES).all()
