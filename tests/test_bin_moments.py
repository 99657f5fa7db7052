"""Bin moments (phk_bin_moments / HipEngine.bin_moments / PSMCKernel.bin_moments / phlash_amd.tmrca_band).

CPU: the float64 dense oracle against path enumeration (a signed row and an indicator, a missing site, a row's own length inside
a bin); the structured (loop-form) statement of the kernel's arithmetic against the dense oracle on the GPU grid's inputs; the
cumulant identity through the tract oracle; the oracle against its own sampled paths; the ABI's argument check without a
device; the lazy re-export.
GPU: the two moments against the oracle for every compiled K (and a padded one) in both precisions with ragged lens and three
value rows; the identities against shipped code (the marginals at bin = 1, a bin against its sites, v = 0, a constant row, the
cumulants through the tract sweep); ll bitwise phk_posterior's; plans / slabs / repeat calls; sampled paths; whole contigs of
different lengths under several models.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import moment_bars as bars
import moment_oracle as mo
import tract_oracle as to
from test_posterior_decode import F32_GAMMA_BAR, F64_GAMMA_BAR, _bcast, _pp_np, _population, _random_pp, _rows, simulate_with_path
from test_tracts import GRID_B, GRID_BINS, GRID_K, GRID_L, GRID_S, grid_sets

GRID_VALUES = ("monotone", "indicator", "signed")


# ------------------------------------------------------------------------------------------------- shared inputs
def grid_values(K):
    """-> {name: [B, K] or [K]}, all within [-1, 1]: a centred monotone row per particle ((k - m - b) / (m + b), m the middle
    state), an indicator (K/4 <= k < 3K/4 + b) and a random signed row (one row for all particles: the stride-0 form)."""
    k = np.arange(K)
    mid = (K - 1) / 2
    rng = np.random.default_rng(70 + K)
    v = {
        "monotone": np.stack([(k - mid - b) / (mid + b) for b in range(GRID_B)]),
        "indicator": np.stack([((k >= K // 4) & (k < (3 * K) // 4 + b)).astype(float) for b in range(GRID_B)]),
        "signed": rng.uniform(-1.0, 1.0, K),
    }
    for a in v.values():
        assert np.abs(a).max() <= 1.0
        a.setflags(write=False)
    return v


def _rows_of(v, b):
    """the three value rows of particle b, [3, K]"""
    return np.stack([v[n] if v[n].ndim == 1 else v[n][b] for n in GRID_VALUES])


@functools.lru_cache(maxsize=None)
def grid_oracle(K):
    """-> {(set, layout): ({bin: (m1, m2), each [3 rows, B, S, nbin]}, ll [B, S])} of the dense float64 oracle, once per K"""
    pp = _population(K, GRID_B, seed=K)
    pc = _population(K, GRID_B * GRID_S, seed=1000 + K)  # one model per (particle, chunk), all different
    v = grid_values(K)
    out = {}
    for i, (rows, W, lens) in enumerate(grid_sets()):
        for layout in ("bcast", "chunk"):
            M = {bin: tuple(np.zeros((3, GRID_B, GRID_S, (GRID_L - W + bin - 1) // bin)) for _ in range(2)) for bin in GRID_BINS}
            ll = np.empty((GRID_B, GRID_S))
            for b in range(GRID_B):
                for s in range(GRID_S):
                    q = _pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * GRID_S + s)
                    m1, m2, ll[b, s] = mo.dense(q, rows[s], _rows_of(v, b), W, GRID_BINS, int(lens[s]))
                    for bin, a1, a2 in zip(GRID_BINS, m1, m2):
                        M[bin][0][:, b, s] = a1
                        M[bin][1][:, b, s] = a2
            for pair in M.values():
                for a in pair:
                    a.setflags(write=False)
            out[i, layout] = (M, ll)
    return out


def _err(x, ref):
    """the grid's metric: max |x - ref| / max(1, |ref|)"""
    return float((np.abs(x - ref) / np.maximum(1.0, np.abs(ref))).max())


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K,L,W,bin", [(2, 8, 0, 3), (3, 7, 1, 3), (4, 6, 0, 1), (4, 6, 1, 3), (3, 8, 1, 1)])
def test_oracle_against_path_enumeration(K, L, W, bin):
    rng = np.random.default_rng(K * 100 + L * 10 + W + bin)
    pp = _random_pp(K, rng)
    data = rng.integers(-1, 2, size=L)
    data[0] = 1  # a het at site 0
    data[L // 2] = -1  # a missing site mid-row
    ind = (np.arange(K) < max(1, K // 2)).astype(float)  # an indicator
    signed = rng.uniform(-1.0, 1.0, K)  # a signed row
    length = W + bin + 1 if bin > 1 else L - 2  # ends inside the second bin / leaves bins without a site of the row's own
    nb = (L - W + bin - 1) // bin
    worst = 0.0
    for v in (ind, signed):
        for n in (None, length):
            m1, m2, ll = mo.dense(pp, data, v, W, bin, n)
            b1, b2 = mo.bruteforce(pp, data, v, W, bin, n)
            assert m1.shape == m2.shape == b1.shape == b2.shape == (nb,)
            worst = max(worst, float(np.abs(m1 - b1).max()), float(np.abs(m2 - b2).max()))
            assert (m2 - m1 * m1 >= -1e-14).all()
            if n is not None:
                empty = (n - W + bin - 1) // bin
                assert not m1[empty:].any() and not m2[empty:].any() and m2[:empty].all()
    print(f"bin-moment oracle vs path enumeration K={K} L={L} W={W} bin={bin}: max |diff| = {worst:.2e}")
    assert worst < 1e-13
    # several value rows and bin sizes in one pass are the single calls
    many1, many2, _ = mo.dense(pp, data, np.stack([ind, signed]), W, (1, bin), length)
    for g, bn in enumerate((1, bin)):
        for j, v in enumerate((ind, signed)):
            a1, a2, _ = mo.dense(pp, data, v, W, bn, length)
            np.testing.assert_allclose(many1[g][j], a1, rtol=0, atol=1e-14)
            np.testing.assert_allclose(many2[g][j], a2, rtol=0, atol=1e-14)
    import posterior_oracle as po

    _, llb = po.bruteforce(pp, data, W)
    assert abs(ll - llb) < 1e-12 * abs(llb) + 1e-13
    # v = 0: exact zeros; the indicator of every state: S = n, exactly known
    z1, z2, _ = mo.dense(pp, data, np.zeros(K), W, bin)
    assert not z1.any() and not z2.any()
    o1, o2, _ = mo.dense(pp, data, np.ones(K), W, bin)
    n = np.array([e - s + 1 for _, s, e in mo._bins(L, W, bin)], float)
    np.testing.assert_allclose(o1, n, rtol=1e-13)
    np.testing.assert_allclose(o2, n * n, rtol=1e-13)


@functools.lru_cache(maxsize=None)
def structured_floor(K):
    """the structured float64 statement against the dense oracle on the GPU grid's inputs (every particle and row of both sets
    in both parameter layouts, the grid's value rows, bins and lens), in the GPU grid's own metrics -> (m1, m2)"""
    pp = _population(K, GRID_B, seed=K)
    pc = _population(K, GRID_B * GRID_S, seed=1000 + K)
    v = grid_values(K)
    w1 = w2 = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        for layout in ("bcast", "chunk"):
            M, _ = grid_oracle(K)[i, layout]
            for b in range(GRID_B):
                for s in range(GRID_S):
                    q = _pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * GRID_S + s)
                    s1, s2 = mo.structured(q, rows[s], _rows_of(v, b), W, GRID_BINS, int(lens[s]))
                    for bin, a1, a2 in zip(GRID_BINS, s1, s2):
                        w1 = max(w1, _err(a1, M[bin][0][:, b, s]))
                        w2 = max(w2, _err(a2, M[bin][1][:, b, s]))
    return w1, w2


@pytest.mark.parametrize("K", GRID_K)
def test_structured_statement_against_the_dense_oracle(K):
    """The kernel's form in float64 loops (folded factors, the adjoint mat-vec's running sums, one power-of-two rescale shared
    by beta, q1 and q2, x2 = w2 + v (w1 + x1)) against the dense oracle: the float64 rounding floor the GPU bars are judged
    against (moment_bars.STRUCTURED_FLOOR)."""
    w1, w2 = structured_floor(K)
    print(f"PARITY bin moments structured-vs-dense K={K}: m1 {w1:.3e}  m2 {w2:.3e}")
    assert max(w1, w2) < bars.STRUCTURED_FLOOR_BAR, (w1, w2)


def test_float64_bar_is_ten_floors_and_float32_bars_five_times_measured():
    assert bars.F64_MOMENT_BAR == 10 * bars.STRUCTURED_FLOOR
    assert bars.STRUCTURED_FLOOR == max(max(m) for m in bars.STRUCTURED_MEASURED.values())
    assert set(bars.F32_MOMENT_BAR) == set(GRID_K)
    for K in GRID_K:
        assert bars.F32_MOMENT_BAR[K] == 5 * max(bars.F32_MEASURED[K])
    assert bars.CUMULANT_M1_BAR == 10 * bars.CUMULANT_M1_MEASURED and bars.CUMULANT_VAR_BAR == 10 * bars.CUMULANT_VAR_MEASURED


def _own_sites(L, W, bin, length):
    """own sites of every bin of the scored sites W .. L - 1 of a row of ``length`` sites"""
    nb = (L - W + bin - 1) // bin
    return np.clip(min(length, L) - W - np.arange(nb) * bin, 0, bin).astype(float)


def cumulants(tract, v, n, h):
    """(m1, var) by central differences of K(l) = log E[exp(l S) | o] at l = +-h.  ``tract(m)``: E[prod m(z_t) | o] per bin for a
    weight row m in [0, 1]; v in [0, 1]; n the own sites per bin.  exp(-h v) gives K(-h); exp(h (v - 1)) gives K(h) - h n."""
    km = np.log(tract(np.exp(-h * v)))
    kp = np.log(tract(np.exp(h * (v - 1.0)))) + h * n
    return (kp - km) / (2 * h), (kp + km) / (h * h)


CUM_CASES = [(K, bin) for K in (4, 16) for bin in (7, 100)]


@functools.lru_cache(maxsize=None)
def cumulant_inputs(K):
    """-> (model, row, value row in [0, 1]) of the cumulant tests: particle 0 and row 0 of the grid's first set, L = 700"""
    rows, W, _ = grid_sets()[0]
    assert W == 0
    return _pp_np(_population(K, GRID_B, seed=K), 0), rows[0], np.linspace(0.0, 1.0, K) ** 2


@pytest.mark.parametrize("K,bin", CUM_CASES)
def test_cumulant_identity_through_the_tract_oracle(K, bin):
    """m1 and m2 - m1^2 are the first two derivatives at 0 of the log of what the tract sweep computes: two code paths that
    share no recursion.  Both sides float64 oracles here; the measured distance is the truncation of the differences."""
    q, row, v = cumulant_inputs(K)
    m1, m2, _ = mo.dense(q, row, v, 0, bin)
    n = _own_sites(GRID_L, 0, bin, GRID_L)
    c1, c2 = cumulants(lambda m: to.dense(q, row, m, 0, bin)[0], v, n, bars.CUMULANT_H)
    var = m2 - m1 * m1
    e1, e2 = _err(c1, m1), _err(c2, var)
    print(f"PARITY bin moments cumulant identity (oracles) K={K} bin={bin}: m1 {e1:.3e}  var {e2:.3e}  (largest var {var.max():.3g})")
    assert var.max() > 0
    assert e1 < bars.CUMULANT_M1_BAR and e2 < bars.CUMULANT_VAR_BAR, (e1, e2)


def test_phk_bin_moments_rejects_a_null_handle_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_bin_moments" in _lib.SIGNATURES
    # (on a thread of its own: the library's last-error string is per thread, and test_layout, which runs later in this
    # process, expects the main thread's to be empty still)
    import threading

    got = []

    def call():
        rc = lib.phk_bin_moments(None, None, 0, 0, None, None, 1, 1, 0, 1, None, 0, None, None, None, None, None)
        got.append((rc, lib.phk_last_error()))

    t = threading.Thread(target=call)
    t.start()
    t.join()
    assert got[0][0] == _lib.PHK_EINVAL
    assert b"NULL" in got[0][1]


def test_tmrca_band_is_lazy_and_has_no_cpu_fallback(monkeypatch):
    import phlash_amd

    f = phlash_amd.tmrca_band
    from phlash_amd.decode import TmrcaBand, tmrca_band

    assert f is tmrca_band and phlash_amd.TmrcaBand is TmrcaBand
    assert TmrcaBand._fields == ("mean", "sd", "sd_within", "sd_between")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dm = phlash_amd.DemographicModel.default("4*1", 1e-4, 1e-4)
    data = np.zeros((1, 50), dtype=np.int8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        tmrca_band(dm, data)


SMP_K, SMP_ROWS, SMP_SITES, SMP_BIN, SMP_N, SMP_DATA_SEED, SMP_SEED = 16, 2, 600, 50, 4000, 21, 11


@functools.lru_cache(maxsize=None)
def sampled():
    """-> (data, dm, the states' expected coalescence times, the float64 oracle's mean and variance of the bin sums
    [rows, nbin]) of the path-sampling test"""
    from phlash_amd.params import PSMCParams

    data, _, dm = simulate_with_path(SMP_K, SMP_ROWS, SMP_SITES, seed=SMP_DATA_SEED, theta=0.05, rho=0.05)
    ect = np.asarray(torch.as_tensor(dm.eta.ect(), dtype=torch.float64).numpy(), float).reshape(SMP_K)
    pp = PSMCParams.from_dm(dm)
    q = _pp_np(PSMCParams(*(torch.as_tensor(a)[None] for a in pp)), 0)
    sc = np.abs(ect).max()
    mom = [mo.dense(q, data[s], ect / sc, 0, SMP_BIN) for s in range(SMP_ROWS)]
    m1 = np.stack([m[0] for m in mom])
    m2 = np.stack([m[1] for m in mom])
    return data, dm, ect, q, sc * m1, sc * sc * (m2 - m1 * m1)


def sample_scores(S, mean, var):
    """S [rows, n, nbin], the draws' bin sums -> (|sample mean - mean| in standard errors sqrt(var / n), |sample variance - var|
    in standard errors formed from the draws' own fourth central moment)"""
    n = S.shape[1]
    d = S - S.mean(1, keepdims=True)
    s2 = (d * d).sum(1) / (n - 1)
    mu4 = (d ** 4).mean(1)
    se_var = np.sqrt(np.maximum(mu4 - s2 * s2, 0.0) / n)
    return np.abs(S.mean(1) - mean) / np.sqrt(var / n), np.abs(s2 - var) / se_var


def test_oracle_against_its_own_sampled_paths():
    """the case of the GPU's path-sampling test, on the CPU: the dense oracle's moments against 4,000 draws of the sampling
    oracle under the same seed.  No bin is excused."""
    import sampling_oracle as so

    data, _, ect, q, mean, var = sampled()
    S = np.stack([ect[so.sample(q, data[s], 0, s, SMP_N, SMP_SEED)[0]].reshape(SMP_N, SMP_SITES // SMP_BIN, SMP_BIN).sum(-1)
                  for s in range(SMP_ROWS)])
    z1, z2 = sample_scores(S, mean, var)
    print(f"oracle vs its own draws: worst mean {z1.max():.2f} se, worst variance {z2.max():.2f} se; sd of S / mean {np.round(np.sqrt(var) / mean, 2)[0].tolist()}")
    assert mean.shape == (SMP_ROWS, SMP_SITES // SMP_BIN) and (var > 0).all()
    assert (z1 <= 5).all() and (z2 <= 5).all()


# ------------------------------------------------------------------------------------------------- GPU
def _np(x):
    return x.double().cpu().numpy()


def _chunk(pc, B, S, K):
    from phlash_amd.params import PSMCParams

    return PSMCParams(*(torch.as_tensor(a).reshape(B, S, K).contiguous() for a in pc))


def _raw(kern, q, inds, v, bin, lens=None):
    """the kernel's own moments of a row that already lies in [-1, 1] (``PSMCKernel.bin_moments`` centres and scales first)
    -> (ll, m1, m2) as numpy / torch: ll stays a tensor"""
    pa, idx, _, _ = kern._model_inputs(q, inds)
    vt = torch.as_tensor(np.array(v, dtype=float), dtype=torch.float64, device=kern.device)
    ll, m1, m2 = kern._eng.bin_moments(pa, idx, vt, warmup=kern.overlap, bin=bin, lens=kern._lens_tensor(lens))
    assert not kern._eng.underflow_risk()
    assert m1.dtype == m2.dtype == torch.float64
    return ll, m1, m2


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
@pytest.mark.parametrize("K", GRID_K)
def test_moments_against_the_oracle(K, dbl):
    from phlash_amd.kernel import get_kernel

    B, S = GRID_B, GRID_S
    pp = _population(K, B, seed=K)
    pc = _population(K, B * S, seed=1000 + K)
    v = grid_values(K)
    w1 = w2 = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        for layout in ("bcast", "chunk"):
            M, LL = grid_oracle(K)[i, layout]
            q = _bcast(pp) if layout == "bcast" else _chunk(pc, B, S, K)
            for bin in GRID_BINS:
                n = GRID_L - W
                nb = M[bin][0].shape[-1]
                empty = np.array([[min((k + 1) * bin, n, int(lens[s]) - W) <= k * bin for k in range(nb)] for s in range(S)])
                assert empty.any()
                for j, name in enumerate(GRID_VALUES):
                    ll, m1, m2 = _raw(kern, q, np.arange(S), v[name], bin, lens)
                    m1, m2 = _np(m1), _np(m2)
                    r1, r2 = M[bin][0][j], M[bin][1][j]
                    assert m1.shape == m2.shape == r1.shape
                    assert np.isfinite(m1).all() and np.isfinite(m2).all()
                    w1, w2 = max(w1, _err(m1, r1)), max(w2, _err(m2, r2))
                    # a bin without a site of the row's own is 0, exactly; every other bin of these rows has a second moment
                    assert not m1[:, empty].any() and not m2[:, empty].any() and not r2[:, empty].any()
                    assert (r2[:, ~empty] > 0).all()
                    rel = np.abs(ll.cpu().numpy() / LL - 1).max()
                    assert rel < (1e-12 if dbl else 1e-5), (bin, layout, W, rel)
    print(f"PARITY bin moments K={K} {'f64' if dbl else 'f32'}: m1 {w1:.3e}  m2 {w2:.3e}")
    assert max(w1, w2) < (bars.F64_MOMENT_BAR if dbl else bars.F32_MOMENT_BAR[K]), (w1, w2)


def _kernel16(dbl=False, S=4, L=5000, W=200, seed=5):
    from phlash_amd.kernel import get_kernel

    rows = _rows(S, L, seed=seed, het=0.05, run=300)
    return rows, get_kernel(16, rows, double_precision=dbl, overlap=W)


def _bar16(dbl):
    return bars.F64_MOMENT_BAR if dbl else bars.F32_MOMENT_BAR[16]


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_single_sites_and_bin_sums_against_phk_posteriors_marginals(dbl):
    """bin = 1: m1 = sum_k v_k gamma_t(k) and m2 = sum_k v_k^2 gamma_t(k); any bin: m1 is the sum of its sites'.  Tolerances
    from the two sides' own bars against the exact values: the moment bar (in units of max(1, |.|), 1 at a single site) plus
    sum_k |v_k| times the marginals' bar; for a bin of n sites the moment bar on the bin plus n times the sites'."""
    rows, kern = _kernel16(dbl)
    q = _population(16, 3, seed=2)
    pp = _bcast(q)
    inds = np.arange(4)
    g = kern.posterior(pp, inds, bin=1).marginals.double()  # [B, S, n, K]
    bar, gbar = _bar16(dbl), (F64_GAMMA_BAR if dbl else F32_GAMMA_BAR)
    for name, v in grid_values(16).items():
        v = v if v.ndim == 1 else np.concatenate([v, v[:1]])  # (three particles here: a row each)
        _, m1, m2 = _raw(kern, pp, inds, v, 1)
        vt = torch.tensor(v, dtype=torch.float64, device=g.device)
        vt = vt[:, None, None, :] if vt.ndim == 2 else vt
        e1 = float((m1 - (g * vt).sum(-1)).abs().max())
        e2 = float((m2 - (g * vt * vt).sum(-1)).abs().max())
        tol = bar + float(np.abs(v).sum(-1).max()) * gbar
        print(f"PARITY bin moments marginal identity {'f64' if dbl else 'f32'} ({name}): m1 {e1:.2e}  m2 {e2:.2e}  (tolerance {tol:.2e})")
        assert e1 < tol and e2 < tol
        n = m1.shape[-1]
        for bin in (7, 100):
            _, b1, _ = _raw(kern, pp, inds, v, bin)
            nb = b1.shape[-1]
            pad = torch.zeros(m1.shape[:-1] + (nb * bin,), dtype=torch.float64, device=m1.device)
            pad[..., :n] = m1
            ref = pad.reshape(m1.shape[:-1] + (nb, bin)).sum(-1)
            err = float(((b1 - ref).abs() / ref.abs().clamp(min=1.0)).max())
            print(f"PARITY bin moments bin {bin} vs the sum of its sites {'f64' if dbl else 'f32'} ({name}): {err:.2e}  (tolerance {(bin + 1) * bar:.2e})")
            assert err < (bin + 1) * bar


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_zero_and_constant_rows_are_exact(dbl):
    rows, kern = _kernel16(dbl)
    pp = _bcast(_population(16, 3, seed=2))
    lens = np.array([5000, 4321, 5000, 777])
    W = kern.overlap
    for bin in (1, 7, 600):
        _, m1, m2 = _raw(kern, pp, np.arange(4), np.zeros(16), bin, lens)
        assert not bool(m1.any()) and not bool(m2.any())
        # a row that is constant over the states: centring makes it zero, so the variance is exactly 0 and the mean is c n
        out = kern.bin_moments(pp, np.arange(4), values=np.full(16, 3.25), bin=bin, lens=lens)
        n = np.stack([_own_sites(5000, W, bin, int(x)) for x in lens])
        assert not bool(out.var.any()) and not bool(out.m1.any()) and not bool(out.m2.any())
        assert out.mean.dtype == out.var.dtype == torch.float64
        assert np.array_equal(_np(out.mean), np.broadcast_to(3.25 * n, out.mean.shape))
        assert (n == 0).any()
        # a general row: bins without a site of the row's own are exactly 0 in every output
        out = kern.bin_moments(pp, np.arange(4), values=np.linspace(2.0, 9.0, 16), bin=bin, lens=lens)
        for x in (out.mean, out.var, out.m1, out.m2):
            assert not _np(x)[:, n == 0].any()
        assert (_np(out.mean)[:, n > 0] > 2.0).all() and (_np(out.var) >= 0).all()


@pytest.mark.gpu
def test_ll_is_bitwise_phk_posteriors():
    rows, kern = _kernel16(False)
    pp = _bcast(_population(16, 3, seed=2))
    inds = np.arange(4)
    v = grid_values(16)["signed"]
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        kern._eng.set_plan(*plan)
        a = kern.bin_moments(pp, inds, values=v, bin=7).ll
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
    v = np.stack([(k - 7.5 - b) / (7.5 + b) for b in range(3)])  # a row per particle: slabs must offset it
    same = lambda x, y: all(torch.equal(p, q) for p, q in zip(x, y))  # noqa: E731
    ll0, g0 = kern(pp, inds, grad=True)  # the gradient call before any moment call
    plan0 = eng.get_plan()
    a = _raw(kern, pp, inds, v, 7, lens)
    b = _raw(kern, pp, inds, v, 7, lens)
    assert same(a, b)
    ll1, g1 = kern(pp, inds, grad=True)
    assert torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert eng.get_plan() == plan0
    # bins: 7 straddles block, segment and unit edges; 600 is larger than a segment of 512 sites; W = 200 lies inside a block
    # of 16 sites (the segmented plan's)
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        for bin in (7, 600):
            eng.set_plan(*plan)  # (a slab is a launch shape of its own: fix the plan so that both runs use the same one)
            a = _raw(kern, pp, inds, v, bin, lens)
            eng.set_workspace_limit(1 << 17)  # three sequences per slab
            c = _raw(kern, pp, inds, v, bin, lens)
            eng.set_workspace_limit(1 << 40)
            assert same(a, c), (plan, bin)
    for bin in (7, 600):
        eng.set_plan(0, 4, 8, 4, 0)
        _, s1, s2 = _raw(kern, pp, inds, v, bin, lens)
        eng.set_plan(1, 4, 16, 4, 4)
        assert eng.get_plan()["segmented"] == 1
        _, g1_, g2_ = _raw(kern, pp, inds, v, bin, lens)
        e1, e2 = _err(_np(g1_), _np(s1)), _err(_np(g2_), _np(s2))
        print(f"serial vs segmented plan, bin {bin}: m1 {e1:.2e}  m2 {e2:.2e}")
        assert max(e1, e2) < 2 * bars.F32_MOMENT_BAR[16]  # (each within the bar of the exact value)


@pytest.mark.gpu
@pytest.mark.parametrize("K,bin", CUM_CASES)
def test_cumulant_identity_through_the_shipped_tract_sweep(K, bin):
    """float64: the central differences of the log of PSMCKernel.tracts at h = 1e-4 against the moment sweep's m1 and m2 - m1^2"""
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    q, row, v = cumulant_inputs(K)
    kern = get_kernel(K, row[None], double_precision=True, overlap=0)
    pp = PSMCParams(**{f: torch.as_tensor(np.asarray(getattr(q, f))) for f in PSMCParams._fields})
    _, m1, m2 = _raw(kern, pp, 0, v, bin)
    m1, m2 = _np(m1), _np(m2)
    n = _own_sites(GRID_L, 0, bin, GRID_L)
    c1, c2 = cumulants(lambda m: _np(kern.tracts(pp, 0, weights=m, bin=bin).prob), v, n, bars.CUMULANT_H)
    var = m2 - m1 * m1
    e1, e2 = _err(c1, m1), _err(c2, var)
    print(f"PARITY bin moments cumulant identity (tract sweep, f64) K={K} bin={bin}: m1 {e1:.3e}  var {e2:.3e}")
    assert e1 < bars.CUMULANT_M1_BAR and e2 < bars.CUMULANT_VAR_BAR, (e1, e2)


@pytest.mark.gpu
def test_sampled_paths_have_the_mean_and_the_variance_the_moments_say():
    """K = 16 float32, one model, 2 rows x 600 windows, bin = 50, 4,000 draws, the states' expected coalescence times: in every
    bin the draws' mean of S within 5 sqrt(var / n) of the kernel's mean and the draws' variance within 5 standard errors (from
    their own fourth moment) of the kernel's variance."""
    from phlash_amd.kernel import get_kernel

    data, dm, ect, _, mean, var = sampled()
    kern = get_kernel(SMP_K, data, double_precision=False)
    inds = np.arange(SMP_ROWS)
    out = kern.bin_moments(dm, inds, values=ect, bin=SMP_BIN)
    km, kv = _np(out.mean), _np(out.var)
    paths = kern.sample_paths(dm, inds, n_samples=SMP_N, seed=SMP_SEED).paths  # [rows, n, L] uint8
    assert paths.shape == (SMP_ROWS, SMP_N, SMP_SITES)
    S = _np(torch.as_tensor(ect, device=paths.device)[paths.long()].reshape(SMP_ROWS, SMP_N, SMP_SITES // SMP_BIN, SMP_BIN).sum(-1))
    z1, z2 = sample_scores(S, km, kv)
    print(f"kernel vs oracle: mean {np.abs(km / mean - 1).max():.2e}, variance {np.abs(kv / var - 1).max():.2e} (relative); "
          f"sampled paths: worst mean {z1.max():.2f} se, worst variance {z2.max():.2f} se")
    assert (z1 <= 5).all(), z1
    assert (z2 <= 5).all(), z2


BAND_WS, BAND_BIN = 100, 10


@functools.lru_cache(maxsize=None)
def band_case():
    """-> (dms, contigs, per-model oracle of the bin-mean TMRCA: mean and variance [3 models, 2 rows, 60 bins], their tolerances)
    of the tmrca_band test: the path-sampling test's rows as two contigs of 345 and 600 windows under three size histories"""
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel

    data, dm, _, _, _, _ = sampled()
    dms = [DemographicModel(eta=dm.eta._replace(c=dm.eta.c * f), theta=dm.theta / BAND_WS, rho=dm.rho / BAND_WS) for f in (1.0, 1.5, 0.7)]
    lens = (345, SMP_SITES)  # 345 windows end inside a bin of 10 and inside a block
    nb = SMP_SITES // BAND_BIN
    mu, var, tm, tv = (np.zeros((3, 2, nb)) for _ in range(4))
    bar = bars.F32_MOMENT_BAR[SMP_K]
    for b, d in enumerate(dms):
        per = DemographicModel(eta=d.eta, theta=float(d.theta) * BAND_WS, rho=float(d.rho) * BAND_WS)
        pp = PSMCParams.from_dm(per)
        q = _pp_np(PSMCParams(*(torch.as_tensor(a)[None] for a in pp)), 0)
        ect = np.asarray(torch.as_tensor(d.eta.ect(), dtype=torch.float64).numpy(), float).reshape(SMP_K)
        c = float((q.pi * ect).sum() / q.pi.sum())
        s = float(np.abs(ect - c).max())
        for r, n_own in enumerate(lens):
            row = np.full(SMP_SITES, -1, dtype=np.int8)
            row[:n_own] = data[r, :n_own]
            m1, m2, _ = mo.dense(q, row, (ect - c) / s, 0, BAND_BIN, n_own)
            n = np.maximum(_own_sites(SMP_SITES, 0, BAND_BIN, n_own), 1.0)
            mu[b, r] = (s * m1 + c * n) / n
            var[b, r] = s * s * (m2 - m1 * m1) / (n * n)
            # what the float32 bars of m1 and m2 allow: |d mean| <= s bar max(1, |m1|) / n, |d var| <= s^2 bar (max(1, m2) + 2 |m1| max(1, |m1|)) / n^2
            tm[b, r] = s * bar * np.maximum(1.0, np.abs(m1)) / n
            tv[b, r] = s * s * bar * (np.maximum(1.0, m2) + 2 * np.abs(m1) * np.maximum(1.0, np.abs(m1))) / (n * n)
    return dms, [data[:1, :345], data[1:, :]], mu, var, tm, tv


@pytest.mark.gpu
def test_tmrca_band_on_ragged_contigs_under_three_models():
    import phlash_amd

    dms, contigs, mu, var, tm, tv = band_case()
    band = phlash_amd.tmrca_band(dms, contigs, window_size=BAND_WS, bin=BAND_BIN)
    assert isinstance(band, phlash_amd.TmrcaBand)
    shapes = [(1, 35), (1, 60)]
    for t in band:
        assert [tuple(x.shape) for x in t] == shapes and all(x.dtype == torch.float64 for x in t)
    for r, nb in enumerate((35, 60)):
        mean, sd, sw, sb = (_np(t[r])[0] for t in band)
        # the mean against the shipped TMRCA track of the contig alone (padded beside a longer contig, posterior_tmrca averages
        # a partial last bin over the padding as well: it takes no lens)
        p = _np(phlash_amd.posterior_tmrca(dms, contigs[r], window_size=BAND_WS, bin=BAND_BIN))[0]
        assert p.shape == mean.shape
        err = float(np.abs(mean - p).max() / np.abs(p).max())
        print(f"PARITY tmrca_band contig {r}: max |mean - posterior_tmrca| / max = {err:.3e}")
        assert err < bars.BAND_MEAN_BAR, err
        # the parts against the oracle composed on the host, within what the float32 bars of m1 and m2 allow
        o_mean = mu[:, r, :nb].mean(0)
        o_within = var[:, r, :nb].mean(0)
        o_between = ((mu[:, r, :nb] - o_mean) ** 2).mean(0)
        t_mean = tm[:, r, :nb].max(0)
        t_between = (2 * np.abs(mu[:, r, :nb] - o_mean) * 2 * t_mean).mean(0) + (2 * t_mean) ** 2
        e = (np.abs(mean - o_mean) / t_mean).max(), (np.abs(sw ** 2 - o_within) / tv[:, r, :nb].mean(0)).max(), (np.abs(sb ** 2 - o_between) / t_between).max()
        print(f"tmrca_band contig {r} vs oracle, in units of the tolerance: mean {e[0]:.2f}  within {e[1]:.2f}  between {e[2]:.2f}; "
              f"sd / mean up to {(sd / mean).max():.2f}, sd_between / sd up to {(sb / sd).max():.2f}")
        assert max(e) < 1, e
        assert (sw > 0).all() and (sb > 0).all()
        np.testing.assert_allclose(sd ** 2, sw ** 2 + sb ** 2, rtol=1e-12, atol=0)
    # one model: nothing between
    one = phlash_amd.tmrca_band(dms[0], contigs[1], window_size=BAND_WS, bin=BAND_BIN)
    assert not bool(one.sd_between.any()) and torch.equal(one.sd, one.sd_within)
    # an indicator row: the share of a bin's windows inside a TMRCA range lies in [0, 1]
    ind = (np.arange(SMP_K) < 9).astype(float)
    share = phlash_amd.tmrca_band(dms, contigs[1], window_size=BAND_WS, bin=BAND_BIN, values=ind)
    assert float(share.mean.min()) >= 0 and float(share.mean.max()) <= 1 + 1e-6 and float(share.sd.max()) <= 0.5 + 1e-6
