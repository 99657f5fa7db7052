"""Local likelihood-ratio scans (phk_local_ratio / HipEngine.local_ratio / PSMCKernel.local_ratio / phlash_amd.local_scan).

CPU: the float64 dense oracle against path enumeration (a missing site, a row's own length inside a bin); its identities (a
whole-row bin is a difference of log-likelihoods, the tract case, the block-out case, alternative = fitted); the structured
(loop-form) statement of the kernel's arithmetic against the dense oracle on the GPU grid's inputs; the planted-region scan; the
ABI's argument check without a device; the lazy re-export.
GPU: the log ratios against the oracle for every compiled K (and a padded one) in both precisions with ragged lens and three
alternatives; plans and rescale intervals; the identities against shipped code (loglik, tracts, predictive, posterior's ll, an
identical alternative); slabs / repeat calls / the plan left alone; the range beyond the linear ratio; flags and errors; and
local_scan end to end.
"""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import local_bars as bars
import local_oracle as lo
from test_posterior_decode import _bcast, _pp_np, _random_pp, _rows
from test_tracts import grid_sets

GRID_K = [4, 8, 12, 16, 32, 64]
GRID_B, GRID_S, GRID_L = 2, 3, 700
GRID_BINS = (1, 7, 100)
GRID_ALTS = ("theta4", "rho4", "ne2")


# ------------------------------------------------------------------------------------------------- shared inputs
def _dms(K, B, seed):
    """B models around the default one (the population of the other sweeps' grids), as one batched DemographicModel"""
    from phlash_amd.synth import particle_population

    tmpl, x = particle_population(K, B, seed=seed, sigma=0.25)
    return tmpl.from_flat(x).to_dm()


def _scaled(dm, what, s):
    from phlash_amd.size_history import DemographicModel, SizeHistory

    if what == "theta":
        return DemographicModel(eta=dm.eta, theta=dm.theta * s, rho=dm.rho)
    if what == "rho":
        return DemographicModel(eta=dm.eta, theta=dm.theta, rho=dm.rho * s)
    return DemographicModel(eta=SizeHistory(t=dm.eta.t, c=dm.eta.c / s), theta=dm.theta, rho=dm.rho)


def _first(dm):
    from phlash_amd.size_history import DemographicModel, SizeHistory

    own = lambda x: x[0] if isinstance(x, torch.Tensor) and x.ndim else x  # noqa: E731  (theta and rho may be shared scalars)
    return DemographicModel(eta=SizeHistory(t=dm.eta.t[0], c=dm.eta.c[0]), theta=own(dm.theta), rho=own(dm.rho))


@functools.lru_cache(maxsize=None)
def grid_models(K):
    """-> {layout: (pp, {name: alt})}, PSMCParams with fields [n, K] (n = B for "bcast", B * S for "chunk": one model per
    (particle, chunk), all different).  The three alternatives: theta x 4 as ONE block for all particles (that of the first
    model; fields [K]), rho / 4 with a block per model, Ne x 2 (c / 2 on the same grid) with a block per model."""
    from phlash_amd.params import PSMCParams

    out = {}
    for layout, n, seed in (("bcast", GRID_B, K), ("chunk", GRID_B * GRID_S, 1000 + K)):
        dm = _dms(K, n, seed)
        alts = {"theta4": PSMCParams.from_dm(_scaled(_first(dm), "theta", 4.0)),
                "rho4": PSMCParams.from_dm(_scaled(dm, "rho", 0.25)),
                "ne2": PSMCParams.from_dm(_scaled(dm, "ne", 2.0))}
        out[layout] = (PSMCParams.from_dm(dm), alts)
    return out


def _alts_np(alts, i):
    """the three alternatives of model i as the oracle's PP"""
    from oracle import psmc_numpy as pn

    one = pn.PP(*(np.asarray(a.numpy(), float) for a in alts["theta4"]))
    return [one, _pp_np(alts["rho4"], i), _pp_np(alts["ne2"], i)]


@functools.lru_cache(maxsize=None)
def grid_oracle(K):
    """-> {(set, layout): ({bin: logratio [3 alternatives, B, S, nbin]}, ll [B, S])} of the dense float64 oracle, once per K"""
    out = {}
    for i, (rows, W, lens) in enumerate(grid_sets()):
        for layout in ("bcast", "chunk"):
            pp, alts = grid_models(K)[layout]
            R = {bin: np.zeros((3, GRID_B, GRID_S, (GRID_L - W + bin - 1) // bin)) for bin in GRID_BINS}
            ll = np.empty((GRID_B, GRID_S))
            for b in range(GRID_B):
                for s in range(GRID_S):
                    m = b if layout == "bcast" else b * GRID_S + s
                    lr, ll[b, s] = lo.dense(_pp_np(pp, m), _alts_np(alts, m), rows[s], W, GRID_BINS, int(lens[s]))
                    for bin, r in zip(GRID_BINS, lr):
                        R[bin][:, b, s] = r
            for r in R.values():
                r.setflags(write=False)
            out[i, layout] = (R, ll)
    return out


def _err(x, ref):
    """the grid's metric: |error| / max(1, |log ratio|)"""
    return np.abs(x - ref) / np.maximum(1.0, np.abs(ref))


def _empty(lens, W, bin, nbin, S):
    n = GRID_L - W
    return np.array([[min((k + 1) * bin, n, int(lens[s]) - W) <= k * bin for k in range(nbin)] for s in range(S)])


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K,L,W,bin", [(2, 8, 0, 3), (3, 7, 1, 3), (4, 6, 0, 1), (4, 6, 1, 3), (3, 8, 1, 1)])
def test_oracle_against_path_enumeration(K, L, W, bin):
    rng = np.random.default_rng(K * 100 + L * 10 + W + bin)
    pp = _random_pp(K, rng)
    alt = _random_pp(K, rng)  # another size history, theta and (through the factors) transition matrix
    data = rng.integers(-1, 2, size=L)
    data[0] = 1  # a het at site 0
    data[L // 2] = -1  # a missing site mid-row
    data[W], data[L - 1] = 1, 0  # (observed sites among the scored ones: all missing, the two models hardly differ)
    length = W + bin + 1 if bin > 1 else L - 2  # ends inside the second bin / leaves bins without a site of the row's own
    for n in (None, length):
        r, ll = lo.dense(pp, alt, data, W, bin, n)
        rb = lo.bruteforce(pp, alt, data, W, bin, n)
        assert r.shape == rb.shape == ((L - W + bin - 1) // bin,)
        np.testing.assert_allclose(r, rb, rtol=0, atol=1e-13)
        if n is None:
            assert np.abs(r).max() > 1e-3  # (the two models differ: the comparison says something)
        else:
            assert not r[(n - W + bin - 1) // bin :].any() and r[: (n - W + bin - 1) // bin].all()
    many, _ = lo.dense(pp, [alt, pp], data, W, (1, bin), length)
    np.testing.assert_allclose(many[1][0], lo.dense(pp, alt, data, W, bin, length)[0], rtol=0, atol=1e-14)
    assert np.abs(many[0][1]).max() <= 1e-14 and np.abs(many[1][1]).max() <= 1e-14  # alternative = fitted
    import posterior_oracle as po

    _, llb = po.bruteforce(pp, data, W)
    assert abs(ll - llb) < 1e-12 * abs(llb) + 1e-13


def _k16(theta=0.03, rho=0.03):
    from oracle import psmc_numpy as pn
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel

    p = PSMCParams.from_dm(DemographicModel.default("16*1", theta, rho))
    return pn.PP(*(np.asarray(a.numpy(), float) for a in p))


def test_oracle_identities():
    """K = 16, L = 700.  One bin over the whole row at W = 0: ll(alternative fields with the fitted pi) - ll(fitted).  Emissions
    multiplied by an indicator on a row without missing windows: tract_oracle.dense.  Emissions set to 1 at bin = 1: minus the
    leave-one-out score at the observed windows.  Alternative = fitted: 0."""
    import posterior_oracle as po
    import predictive_oracle as pr
    import tract_oracle as to

    K, L = 16, 700
    pp, alt = _k16(0.03, 0.03), _k16(0.12, 0.01)
    rng = np.random.default_rng(5)
    full = (rng.random(L) < 0.05).astype(int)  # no missing window
    holes = full.copy()
    holes[rng.integers(0, L, 20)] = -1
    for data in (full, holes):
        r, ll = lo.dense(pp, alt, data, 0, L)
        _, ll0 = po.forward_backward(pp, data, 0)
        _, ll1 = po.forward_backward(alt._replace(pi=pp.pi), data, 0)
        err = abs(r[0] - (ll1 - ll0))
        print(f"whole-row bin {r[0]:.6f} vs ll difference {ll1 - ll0:.6f}: |diff| {err:.2e}")
        assert r.shape == (1,) and abs(ll - ll0) < 1e-12 * abs(ll0)
        assert err < 1e-12  # (two sums of 700 logs of O(1) numbers: 700 x 2.2e-16 x a few)
    m = (np.arange(K) < 10).astype(float)
    for bin in (1, 7, 100):
        r, _ = lo.dense(pp, pp._replace(emis0=pp.emis0 * m, emis1=pp.emis1 * m), full, 37, bin)
        t, _ = to.dense(pp, full, m, 37, bin)
        print(f"tract case, bin {bin}: max |exp(log ratio) - tract| {np.abs(np.exp(r) - t).max():.2e}")
        assert np.abs(np.exp(r) - t).max() < 1e-14
    one = np.ones(K)
    r, _ = lo.dense(pp, pp._replace(emis0=one, emis1=one), holes, 37, 1)
    _, score, _ = pr.loo(pp, holes, 37)
    print(f"block-out case: max |log ratio + score| {np.abs(r + score).max():.2e}")
    assert np.abs(r + score).max() < 1e-13 and not r[holes[37:] < 0].any()
    for bin in (1, 7, 100):
        assert np.abs(lo.dense(pp, pp, holes, 37, bin)[0]).max() <= 1e-14


@functools.lru_cache(maxsize=None)
def structured_floor(K):
    """the structured float64 statement against the dense oracle on the GPU grid's inputs (every particle and row of both sets
    in both parameter layouts, the grid's alternatives, bins and lens), in the GPU grid's own metric"""
    worst = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        for layout in ("bcast", "chunk"):
            pp, alts = grid_models(K)[layout]
            R, _ = grid_oracle(K)[i, layout]
            for b in range(GRID_B):
                for s in range(GRID_S):
                    m = b if layout == "bcast" else b * GRID_S + s
                    lr = lo.structured(_pp_np(pp, m), _alts_np(alts, m), rows[s], W, GRID_BINS, int(lens[s]))
                    for bin, r in zip(GRID_BINS, lr):
                        worst = max(worst, float(_err(r, R[bin][:, b, s]).max()))
    return worst


@pytest.mark.parametrize("K", GRID_K)
def test_structured_statement_against_the_dense_oracle(K):
    """The kernel's form in float64 loops (folded factors per model, the adjoint mat-vec's running sums, beta's power-of-two
    rescale and q's own exponent) against the dense oracle: the float64 rounding floor the GPU bars are judged against
    (local_bars.STRUCTURED_FLOOR)."""
    worst = structured_floor(K)
    print(f"PARITY local ratio structured-vs-dense K={K}: max |err| / max(1, |log ratio|) = {worst:.3e}")
    assert worst < bars.STRUCTURED_FLOOR_BAR, worst


def test_structured_statement_keeps_its_exponent_and_its_exact_zero():
    """what the dense oracle's log scale and the structured statement's integer exponent are for: the 700-window half-het row
    with the emissions removed (log ratio = -ll, 851), and an alternative equal to the fitted model (exactly 0)"""
    pp = _k16(0.01, 0.01)
    data = (np.random.default_rng(3).uniform(size=700) < 0.5).astype(int)
    one = np.ones(16)
    r, ll = lo.dense(pp, pp._replace(emis0=one, emis1=one), data, 0, 700)
    assert abs(r[0] + ll) < 1e-10 and abs(r[0] - 851.08) < 0.01
    rs = lo.structured(pp, pp._replace(emis0=one, emis1=one), data, 0, 700)
    assert abs(rs[0] - r[0]) < 1e-10
    for bin in (1, 100):
        assert not lo.structured(pp, pp, data, 37, bin).any()


def test_float64_bar_is_ten_floors():
    assert bars.F64_LOCAL_BAR <= 10 * bars.STRUCTURED_FLOOR


PLANT_K, PLANT_ROWS, PLANT_L, PLANT_BIN, PLANT_THETA = 16, 8, 1400, 100, 0.03
PLANT_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0)


@functools.lru_cache(maxsize=None)
def planted():
    """8 rows of 1,400 windows under theta = rho = 0.03 per window, windows 500 .. 799 spliced in from rows simulated with
    theta = 0.12: bins 5, 6, 7 of 100 windows have four times the mutation rate"""
    from phlash_amd.synth import simulate_chunks

    d = simulate_chunks(PLANT_K, PLANT_ROWS, PLANT_L, seed=11, theta=PLANT_THETA, rho=PLANT_THETA)
    hot = simulate_chunks(PLANT_K, PLANT_ROWS, PLANT_L, seed=12, theta=4 * PLANT_THETA, rho=PLANT_THETA)
    d[:, 500:800] = hot[:, 500:800]
    d.setflags(write=False)
    return d


def _planted_conditions(composite, scales):
    """composite [nbin, J] over ``scales``: the best scale is >= 2 in exactly bins 5, 6, 7 and <= 1 elsewhere; the summed log
    ratio at scale 4 is positive inside and negative outside"""
    composite = np.asarray(composite)
    sc = np.asarray(scales)
    best = sc[composite.argmax(-1)]
    inside = np.isin(np.arange(composite.shape[0]), (5, 6, 7))
    at4 = composite[:, list(scales).index(4.0)]
    print(f"planted region: best scale per bin {best.tolist()}; summed log ratio at scale 4 {np.round(at4, 1).tolist()}")
    assert composite.shape == (PLANT_L // PLANT_BIN, len(scales))
    assert (best[inside] >= 2).all() and (best[~inside] <= 1).all()
    assert (at4[inside] > 0).all() and (at4[~inside] < 0).all()


def test_planted_region_is_found_by_the_oracle():
    d = planted()
    others = [s for s in PLANT_SCALES if s != 1.0]
    alts = [_k16(PLANT_THETA * s, PLANT_THETA) for s in others]
    comp = np.zeros((PLANT_L // PLANT_BIN, len(PLANT_SCALES)))
    for r in range(PLANT_ROWS):
        lr, _ = lo.dense(_k16(PLANT_THETA, PLANT_THETA), alts, d[r], 0, PLANT_BIN)
        for j, s in enumerate(others):
            comp[:, PLANT_SCALES.index(s)] += lr[j]
    _planted_conditions(comp, PLANT_SCALES)


def test_phk_local_ratio_rejects_a_null_handle_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_local_ratio" in _lib.SIGNATURES
    rc = lib.phk_local_ratio(None, None, 0, 0, None, None, 0, 0, None, None, 1, 1, 0, 1, None, None, None, None)
    assert rc == _lib.PHK_EINVAL
    assert b"NULL" in lib.phk_last_error()


def test_local_scan_is_lazy_and_has_no_cpu_fallback(monkeypatch):
    import phlash_amd

    f = phlash_amd.local_scan
    from phlash_amd.decode import local_scan
    from phlash_amd.kernel import PSMCKernel

    assert f is local_scan and hasattr(PSMCKernel, "local_ratio")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dm = phlash_amd.DemographicModel.default("4*1", 1e-4, 1e-4)
    data = np.zeros((1, 50), dtype=np.int8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        local_scan(dm, data)


# ------------------------------------------------------------------------------------------------- GPU
def _np(x):
    return x.double().cpu().numpy()


def _shaped(p, layout, K):
    """fields [n, K] -> [B, 1, K] ("bcast") or [B, S, K] ("chunk"); fields [K] (one block for everything) stay"""
    from phlash_amd.params import PSMCParams

    if p.d.ndim == 1:
        return p
    if layout == "bcast":
        return _bcast(p)
    return PSMCParams(*(torch.as_tensor(a).reshape(GRID_B, GRID_S, K).contiguous() for a in p))


def _grid_worst(K, dbl, sets=(0, 1), setup=None):
    from phlash_amd.kernel import get_kernel

    S = GRID_S
    worst = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        if i not in sets:
            continue
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        if setup is not None:
            setup(kern._eng)
        for layout in ("bcast", "chunk"):
            R, LL = grid_oracle(K)[i, layout]
            pp, alts = grid_models(K)[layout]
            q = _shaped(pp, layout, K)
            for bin in GRID_BINS:
                empty = _empty(lens, W, bin, R[bin].shape[-1], S)
                assert empty.any()
                for j, name in enumerate(GRID_ALTS):
                    out = kern.local_ratio(q, _shaped(alts[name], layout, K), np.arange(S), bin=bin, lens=lens)
                    assert not kern._eng.underflow_risk()
                    r = _np(out.log_ratio)
                    assert r.shape == R[bin][j].shape and np.isfinite(r).all()
                    worst = max(worst, float(_err(r, R[bin][j]).max()))
                    # a bin without a site of the row's own is 0, exactly
                    assert not r[:, empty].any() and not R[bin][j][:, empty].any()
                    rel = np.abs(out.ll.cpu().numpy() / LL - 1).max()
                    assert rel < (1e-12 if dbl else 1e-5), (bin, layout, W, rel)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
@pytest.mark.parametrize("K", GRID_K)
def test_local_ratio_against_the_oracle(K, dbl):
    worst = _grid_worst(K, dbl)
    print(f"PARITY local ratio K={K} {'f64' if dbl else 'f32'}: max |err| / max(1, |log ratio|) = {worst:.3e}")
    assert worst < (bars.F64_LOCAL_BAR if dbl else bars.F32_LOCAL_BAR), worst


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
@pytest.mark.parametrize("plan", [(0, 4, 8, 4, 0), (1, 4, 16, 4, 4)])
@pytest.mark.parametrize("nrm", [1, 2, 4])
def test_plans_and_rescale_intervals_against_the_oracle(nrm, plan, dbl):
    """K = 16, the second row set (W = 37, runs of missing windows): the serial and the segmented plan at every rescale interval"""

    def setup(eng):
        eng.set_plan(*plan)
        eng.set_rescale_interval(nrm)

    worst = _grid_worst(16, dbl, sets=(1,), setup=setup)
    print(f"PARITY local ratio plan={plan} nrm={nrm} {'f64' if dbl else 'f32'}: max |err| / max(1, |log ratio|) = {worst:.3e}")
    assert worst < (bars.F64_LOCAL_BAR if dbl else bars.F32_LOCAL_BAR), worst


def _kernel16(dbl=False, S=4, L=5000, W=200, seed=5):
    from phlash_amd.kernel import get_kernel

    rows = _rows(S, L, seed=seed, het=0.05, run=300)
    return rows, get_kernel(16, rows, double_precision=dbl, overlap=W)


def _models16(B=3, seed=2):
    """-> (pp, alt) with fields [B, 1, K]: B models and their theta x 2 alternatives"""
    from phlash_amd.params import PSMCParams

    dm = _dms(16, B, seed)
    return _bcast(PSMCParams.from_dm(dm)), _bcast(PSMCParams.from_dm(_scaled(dm, "theta", 2.0)))


@pytest.mark.gpu
def test_whole_row_bin_is_the_likelihood_ratio_of_loglik():
    """One bin of L sites, W = 0, float64, K = 16: log ratio = ll(alternative fields with the fitted pi) - ll(fitted), both from
    the shipped no-gradient call: code that shares only the forward step with the local-ratio sweep."""
    from phlash_amd.kernel import get_kernel

    L = 200
    rng = np.random.default_rng(17)
    data = (rng.random((2, L)) < 0.05).astype(np.int8)
    data[:, 0] = 1
    data[1, 50:60] = -1
    kern = get_kernel(16, data, double_precision=True, overlap=0)
    pp, alt = _models16(2, seed=4)
    out = kern.local_ratio(pp, alt, np.arange(2), bin=L)
    assert out.log_ratio.shape == (2, 2, 1)
    lr = _np(out.log_ratio)[..., 0]
    ll0 = np.asarray(kern(pp, np.arange(2), grad=False).cpu().numpy(), float)
    ll1 = np.asarray(kern(alt._replace(pi=pp.pi), np.arange(2), grad=False).cpu().numpy(), float)
    err = np.abs(lr - (ll1 - ll0)).max()
    print(f"log ratio {lr.tolist()}, ll difference {(ll1 - ll0).tolist()}")
    print(f"PARITY local ratio likelihood-ratio identity: max |log ratio - (ll_alt - ll)| = {err:.3e}")
    assert (np.abs(lr) > 0.5).all()  # (a ratio far from 1: the identity says something)
    assert err < bars.F64_LIKELIHOOD_RATIO_BAR, err


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_tract_case_is_phk_tracts(dbl):
    """emissions multiplied by an indicator, rows without missing windows: exp(log ratio) is PSMCKernel.tracts' probability"""
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    rng = np.random.default_rng(9)
    data = (rng.random((3, 900)) < 0.05).astype(np.int8)
    kern = get_kernel(16, data, double_precision=dbl, overlap=37)
    pp, _ = _models16()
    m = torch.as_tensor((np.arange(16) < 10).astype(float))
    alt = pp._replace(emis0=pp.emis0 * m, emis1=pp.emis1 * m)
    worst = 0.0
    for bin in (1, 7, 100):
        r = _np(kern.local_ratio(pp, PSMCParams(*alt), np.arange(3), bin=bin).log_ratio)
        t = _np(kern.tracts(pp, np.arange(3), weights=m.numpy(), bin=bin).prob)
        worst = max(worst, float(np.abs(np.exp(r) - t).max()))
    print(f"PARITY local ratio tract case {'f64' if dbl else 'f32'}: max |exp(log ratio) - tract| = {worst:.3e}")
    assert worst < (bars.F64_TRACT_CASE_BAR if dbl else bars.F32_TRACT_CASE_BAR), worst


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_block_out_case_is_phk_predictives_score(dbl):
    """emissions set to 1, bin = 1: the log ratio is minus the leave-one-out score PSMCKernel.predictive reports (0 at a missing
    window in both)"""
    rows, kern = _kernel16(dbl)
    pp, _ = _models16()
    one = torch.ones_like(pp.emis0)
    r = _np(kern.local_ratio(pp, pp._replace(emis0=one, emis1=one), np.arange(4), bin=1).log_ratio)
    s = _np(kern.predictive(pp, np.arange(4), bin=1).score)
    err = float(_err(r, -s).max())
    print(f"PARITY local ratio block-out case {'f64' if dbl else 'f32'}: max |log ratio + score| / max(1, |score|) = {err:.3e}")
    assert (np.abs(s) > 1).any()
    # (a missing window has score 0; the log ratio there is 0 up to rounding only: the fitted lane multiplies its folded factors
    # by 1 / emis0 where the alternative's factors never held emis0)
    assert not s[:, rows[:, kern.overlap:] < 0].any()
    assert err < (bars.F64_BLOCK_OUT_BAR if dbl else bars.F32_BLOCK_OUT_BAR), err


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_identical_alternative_gives_exactly_zero(dbl):
    """alternative bit-identical to the fitted block: q is beta bit for bit and its exponent stays 0, so every bin is exactly 0
    -- the own ones and the empty ones -- under both plans"""
    rows, kern = _kernel16(dbl)
    pp, _ = _models16()
    lens = np.array([5000, 4321, 5000, 777])
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        kern._eng.set_plan(*plan)
        for bin in (1, 7, 600):
            r = kern.local_ratio(pp, pp, np.arange(4), bin=bin, lens=lens).log_ratio
            assert r.shape[-1] == (5000 - kern.overlap + bin - 1) // bin
            assert not bool(r.any()), (plan, bin, float(r.abs().max()))


@pytest.mark.gpu
def test_ll_is_bitwise_phk_posteriors():
    rows, kern = _kernel16(False)
    pp, alt = _models16()
    inds = np.arange(4)
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        kern._eng.set_plan(*plan)
        a = kern.local_ratio(pp, alt, inds, bin=7).ll
        b = kern.posterior(pp, inds, bin=7).ll
        assert torch.equal(a, b), (plan, float((a - b).abs().max()))


@pytest.mark.gpu
def test_plans_slabs_and_repeats_are_consistent():
    rows, kern = _kernel16(False)
    eng = kern._eng
    pp, alt = _models16(3, seed=7)  # a block per particle: slabs must offset it
    inds = np.arange(4)
    lens = np.array([5000, 4321, 5000, 777])
    same = lambda x, y: all(torch.equal(p, q) for p, q in zip(x, y))  # noqa: E731
    ll0, g0 = kern(pp, inds, grad=True)  # the gradient call before any local-ratio call
    plan0 = eng.get_plan()
    a = kern.local_ratio(pp, alt, inds, bin=7, lens=lens)
    b = kern.local_ratio(pp, alt, inds, bin=7, lens=lens)
    assert same(a, b)
    ll1, g1 = kern(pp, inds, grad=True)
    assert torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert eng.get_plan() == plan0
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        for bin in (7, 600):
            eng.set_plan(*plan)  # (a slab is a launch shape of its own: fix the plan so that both runs use the same one)
            a = kern.local_ratio(pp, alt, inds, bin=bin, lens=lens)
            eng.set_workspace_limit(1 << 17)  # three sequences per slab
            c = kern.local_ratio(pp, alt, inds, bin=bin, lens=lens)
            eng.set_workspace_limit(1 << 40)
            assert same(a, c), (plan, bin)
    for bin in (7, 600):
        eng.set_plan(0, 4, 8, 4, 0)
        ser = _np(kern.local_ratio(pp, alt, inds, bin=bin, lens=lens).log_ratio)
        eng.set_plan(1, 4, 16, 4, 4)
        assert eng.get_plan()["segmented"] == 1
        seg = _np(kern.local_ratio(pp, alt, inds, bin=bin, lens=lens).log_ratio)
        err = float(_err(seg, ser).max())
        print(f"serial vs segmented plan, bin {bin}: max |diff| / max(1, |log ratio|) {err:.2e}")
        assert err < bars.F32_LOCAL_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_range_beyond_the_linear_ratio(dbl):
    """A 700-window row with half its windows het, K = 16, theta = rho = 0.01, emissions removed.  One whole-row bin: the log
    ratio is -ll = 851.08, beyond what a float64 linear ratio holds; W = 37, bin = 100: 77 .. 114 per bin, beyond float32's
    linear range in most bins.  Both within the grid's bar, and no underflow flag."""
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    data = (np.random.default_rng(3).uniform(size=(1, 700)) < 0.5).astype(np.int8)
    q = _k16(0.01, 0.01)
    one = np.ones(16)
    pp = PSMCParams(*(torch.as_tensor(a) for a in q))
    alt = pp._replace(emis0=torch.as_tensor(one), emis1=torch.as_tensor(one))
    bar = bars.F64_LOCAL_BAR if dbl else bars.F32_LOCAL_BAR
    for W, bin in ((0, 700), (37, 100)):
        ref, ll = lo.dense(q, q._replace(emis0=one, emis1=one), data[0], W, bin)
        kern = get_kernel(16, data, double_precision=dbl, overlap=W)
        out = kern.local_ratio(pp, alt, 0, bin=bin)
        assert not kern._eng.underflow_risk()
        r = _np(out.log_ratio)
        err = float(_err(r, ref).max())
        print(f"range W={W} bin={bin} {'f64' if dbl else 'f32'}: oracle {np.round(ref, 2).tolist()}, max |err| / |log ratio| {err:.3e}")
        assert r.shape == ref.shape and np.isfinite(r).all()
        if bin == 700:
            assert abs(ref[0] + ll) < 1e-9 and abs(ref[0] - 851.08) < 0.01
        else:
            assert ref.min() > 76 and ref.max() < 115 and (ref > 88.8).sum() >= 4
        assert err < bar, err


@pytest.mark.gpu
def test_flags_and_errors():
    from phlash_amd import _lib
    from phlash_amd.params import PSMCParams

    rows, kern = _kernel16(False, S=2, L=600, W=20)
    eng = kern._eng
    pp, alt = _models16(2)
    inds = np.arange(2)
    # an out-of-range lens entry: clamped, and the bad-index flag
    P, A = (torch.stack(list(x), -2).to(kern.device) for x in (pp, alt))
    di = torch.arange(2, device=kern.device)
    for bad in ([600, 20], [601, 600]):
        _, r = eng.local_ratio(P, A, di, warmup=20, bin=7, lens=torch.tensor(bad, device=kern.device))
        assert bool(torch.isfinite(r).all())
        with pytest.raises(AssertionError, match="outside"):
            eng.underflow_risk()
    assert not eng.underflow_risk()
    # an alternative that forbids the data: het emission 0 -> -inf in every bin with an observed het, finite elsewhere, no flag
    dead = PSMCParams(*alt)._replace(emis1=torch.zeros_like(alt.emis1))
    r = _np(kern.local_ratio(pp, dead, inds, bin=7).log_ratio)
    assert not eng.underflow_risk()
    n = 600 - 20
    het = np.array([[(rows[s, 20 + k * 7 : min(20 + (k + 1) * 7, 600)] >= 1).any() for k in range((n + 6) // 7)] for s in range(2)])
    assert het.any() and (~het).any()
    assert np.isneginf(r[:, het]).all() and np.isfinite(r[:, ~het]).all()
    # every PHK_EINVAL case, before anything is enqueued
    lib = _lib.load()
    p32, a32 = P.float().contiguous(), A.float().contiguous()
    ll = torch.empty((2, 2), dtype=torch.float64, device=kern.device)
    out = torch.full((2, 2, 83), 7.0, dtype=torch.float32, device=kern.device)
    sb, ss = 7 * 16, 0
    good = dict(h=eng._h, params=p32.data_ptr(), alt=a32.data_ptr(), inds=di.data_ptr(), W=20, bin=7, ll=ll.data_ptr(), out=out.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.phk_local_ratio(a["h"], a["params"], sb, ss, None, a["alt"], sb, ss, None, a["inds"], 2, 2, a["W"], a["bin"], None,
                                   a["ll"], a["out"], None)

    for kw in (dict(h=None), dict(params=None), dict(alt=None), dict(inds=None), dict(ll=None), dict(bin=0), dict(W=-1), dict(W=601),
               dict(out=None)):
        assert call(**kw) == _lib.PHK_EINVAL, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was enqueued
    assert call() == _lib.PHK_OK
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
    # W = L: no scored site, empty outputs
    assert call(W=600, out=None) == _lib.PHK_OK
    torch.cuda.synchronize()
    assert not bool(ll.any())
    from phlash_amd.kernel import get_kernel

    k2 = get_kernel(16, rows, double_precision=False, overlap=600)
    e = k2.local_ratio(pp, alt, inds, bin=7)
    assert e.log_ratio.shape == (2, 2, 0) and e.ll.shape == (2, 2) and not bool(e.ll.any())


@pytest.mark.gpu
def test_local_scan_finds_the_planted_region():
    import phlash_amd

    ws = 100
    dm = phlash_amd.DemographicModel.default("16*1", PLANT_THETA / ws, PLANT_THETA / ws)
    d = np.array(planted())
    out = phlash_amd.local_scan(dm, d, what="theta", scales=(0.25, 0.5, 2.0, 4.0, 8.0), window_size=ws, bin=PLANT_BIN)
    assert out.scales == PLANT_SCALES
    assert out.log_ratio.shape == (PLANT_ROWS, PLANT_L // PLANT_BIN, 6) and out.log_ratio.dtype == torch.float64
    assert torch.equal(out.composite, out.log_ratio.sum(0))
    assert not bool(out.log_ratio[..., 2].any())  # scale 1: the exact zero column
    _planted_conditions(_np(out.composite), out.scales)
    sc = np.asarray(out.scales)
    assert np.array_equal(_np(out.best), sc[_np(out.composite).argmax(-1)])


@pytest.mark.gpu
def test_local_scan_ragged_contigs_models_and_ne():
    import phlash_amd
    from phlash_amd.kernel import get_kernel
    from phlash_amd.size_history import DemographicModel, SizeHistory

    ws, bin = 100, 10
    d = np.array(planted())[:3, :600]
    base = phlash_amd.DemographicModel.default("16*1", PLANT_THETA / ws, PLANT_THETA / ws)
    dms = [base, DemographicModel(eta=SizeHistory(t=base.eta.t, c=base.eta.c * 1.5), theta=base.theta, rho=base.rho)]
    contigs = [d[:1, :345], d[1:, :]]  # 345 windows end inside a bin of 10 and inside a block
    rag = phlash_amd.local_scan(dms[0], contigs, what="rho", scales=(0.5, 2.0), window_size=ws, bin=bin)
    assert rag.scales == (0.5, 1.0, 2.0)
    assert [tuple(r.shape) for r in rag.log_ratio] == [(1, 35, 3), (2, 60, 3)]
    assert [tuple(c.shape) for c in rag.composite] == [(35, 3), (60, 3)] and [tuple(b.shape) for b in rag.best] == [(35,), (60,)]
    for c, r, comp in zip(contigs, rag.log_ratio, rag.composite):
        alone = phlash_amd.local_scan(dms[0], c, what="rho", scales=(0.5, 2.0), window_size=ws, bin=bin)
        err = float((r - alone.log_ratio).abs().max())
        print(f"contig of {c.shape[1]} windows, padded vs alone: max |diff| {err:.2e}")
        assert err < bars.F32_LOCAL_BAR
        assert torch.equal(comp, r.sum(0)) and not bool(r[..., 1].any()) and bool(r[..., 0].all())
    # the mean over the models of the per-model log ratios
    both = phlash_amd.local_scan(dms, d, what="theta", scales=(2.0,), window_size=ws, bin=bin)
    each = [phlash_amd.local_scan(m, d, what="theta", scales=(2.0,), window_size=ws, bin=bin) for m in dms]
    assert float((both.log_ratio - (each[0].log_ratio + each[1].log_ratio) / 2).abs().max()) < 1e-12
    # "ne": the hand-built model with c / scale on the same grid, through the kernel's own call
    ne = phlash_amd.local_scan(base, d, what="ne", scales=(0.5,), window_size=ws, bin=bin)
    per = DemographicModel(eta=base.eta, theta=base.theta * ws, rho=base.rho * ws)
    hand = DemographicModel(eta=SizeHistory(t=base.eta.t, c=base.eta.c / 0.5), theta=per.theta, rho=per.rho)
    ref = get_kernel(16, d, double_precision=False).local_ratio(per, hand, np.arange(3), bin=bin).log_ratio
    assert ne.scales == (0.5, 1.0) and torch.equal(ne.log_ratio[..., 0], ref.double())
