"""Pair counts (phk_pair_counts / HipEngine.pair_counts / PSMCKernel.pair_counts / phlash_amd.transition_counts), the part that
needs no GPU: the float64 oracle against path enumeration, against the arrivals of the transition oracle and against the number
of own scored sites; the loop-form statement of the kernel's sums against the dense oracle on the GPU grid's inputs (the float64
floor the GPU bars are judged against); the ABI's argument check without a device; the lazy re-export; and the reduction of
``transition_counts`` over contigs and models on a stub kernel object that returns known matrices.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import pair_count_bars as bars
import pair_count_oracle as pco
import transition_oracle as to
from test_posterior_decode import _pp_np, _population, _random_pp, _rows

GRID_K = [4, 8, 12, 16, 32, 64]
GRID_B, GRID_S, GRID_L = 2, 3, 700


# ------------------------------------------------------------------------------------------------- shared inputs
def grid_sets():
    """The two row sets of the oracle grid: (rows, W, lens).  Rows with isolated missing sites (both) and with runs of missing
    windows (the second).  lens: 593 and 437 end inside a block (of 8 and of 16 sites), 1 (W = 0) and 38 (W = 37) are one site past
    W, 700 is L.  The rows keep their data past the own lengths (the mask alone)."""
    r1 = _rows(GRID_S, GRID_L, seed=1)
    r2 = _rows(GRID_S, GRID_L, seed=2, run=120)
    return [(r1, 0, np.array([700, 593, 1])), (r2, 37, np.array([38, 700, 437]))]


@functools.lru_cache(maxsize=None)
def grid_oracle(K):
    """-> {(set, layout): (C [B, S, K, K], ll [B, S])} of the dense float64 oracle at the sets' own lens, computed once per K"""
    pp = _population(K, GRID_B, seed=K)
    pc = _population(K, GRID_B * GRID_S, seed=1000 + K)  # one model per (particle, chunk), all different
    out = {}
    for i, (rows, W, lens) in enumerate(grid_sets()):
        for layout in ("bcast", "chunk"):
            C = np.empty((GRID_B, GRID_S, K, K))
            ll = np.empty((GRID_B, GRID_S))
            for b in range(GRID_B):
                for s in range(GRID_S):
                    q = _pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * GRID_S + s)
                    C[b, s], ll[b, s] = pco.pair_counts(q, rows[s], W, int(lens[s]))
            C.setflags(write=False)
            out[i, layout] = (C, ll)
    return out


# ------------------------------------------------------------------------------------------------- the oracle
def test_oracle_against_path_enumeration():
    K, L = 3, 5
    rng = np.random.default_rng(35)
    pp = _random_pp(K, rng)
    data = np.array([0, 1, 0, -1, 0])  # one het, one missing site
    for W, length in ((0, None), (0, 4), (2, None), (2, 3)):
        C, _ = pco.pair_counts(pp, data, W, length)
        xb = to.bruteforce_pairs(pp, data, W)
        n = (L if length is None else length) - W
        np.testing.assert_allclose(C, xb[:n].sum(0), rtol=0, atol=1e-13)
        assert abs(C.sum() - n) < 1e-13
    # asymmetric: a transposed or permuted matrix is another matrix
    C, _ = pco.pair_counts(pp, data, 0)
    off = C - np.diag(np.diag(C))
    assert np.abs(off - off.T).max() > 0.1 * off.max()


def test_oracle_sums_are_the_arrivals_and_the_site_count():
    rng = np.random.default_rng(6)
    for K, W, length in ((8, 0, 300), (16, 40, 211)):
        pp = _random_pp(K, rng)
        data = (rng.random(300) < 0.05).astype(int)
        data[rng.integers(0, 300, 5)] = -1
        data[100:130] = -1
        C, ll = pco.pair_counts(pp, data, W, length)
        xi, ll2 = to.pair_posteriors(pp, data, W)
        arr = to.arrivals_of(xi)[: length - W].sum(0)  # [3, K]
        np.testing.assert_allclose(np.diag(C), arr[0], rtol=0, atol=1e-11)
        np.testing.assert_allclose(np.triu(C, 1).sum(0), arr[1], rtol=0, atol=1e-11)
        np.testing.assert_allclose(np.tril(C, -1).sum(0), arr[2], rtol=0, atol=1e-11)
        assert abs(C.sum() - (length - W)) < 1e-10
        assert ll == ll2


@pytest.mark.parametrize("K", GRID_K)
def test_loop_form_against_the_dense_oracle(K):
    """The kernel's form in float64 loops (folded factors, raw outer products over Z_t, A applied last) against the dense oracle
    on the GPU grid's inputs (particle 0 of the broadcast layout, every row of both sets), in the tests' metric
    |C - oracle| / max(1, oracle).  Measured: 9.4e-15 at worst (K = 16): the float64 floor the GPU bars are judged against."""
    pp = _population(K, GRID_B, seed=K)
    worst = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        C, _ = grid_oracle(K)[i, "bcast"]
        for s in range(GRID_S):
            worst = max(worst, pco.error(pco.loop_form(_pp_np(pp, 0), rows[s], W, int(lens[s])), C[0, s]))
    print(f"PARITY pair counts loop-form-vs-dense K={K}: max |diff| / max(1, oracle) = {worst:.3e}")
    assert worst < bars.LOOP_FORM_FLOOR_BAR, worst


# ------------------------------------------------------------------------------------------------- the ABI and the package
def test_phk_pair_counts_rejects_a_null_handle_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_pair_counts" in _lib.SIGNATURES
    rc = lib.phk_pair_counts(None, None, 0, 0, None, None, 1, 1, 0, None, None, None, None)
    assert rc == _lib.PHK_EINVAL
    assert b"NULL" in lib.phk_last_error()


def test_transition_counts_is_lazy_and_has_no_cpu_fallback(monkeypatch):
    import phlash_amd

    f = phlash_amd.transition_counts
    from phlash_amd.decode import TransitionCounts, transition_counts

    assert f is transition_counts and phlash_amd.TransitionCounts is TransitionCounts
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dm = phlash_amd.DemographicModel.default("4*1", 1e-4, 1e-4)
    data = np.zeros((1, 50), dtype=np.int8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        transition_counts(dm, data)


def test_transition_counts_reduces_over_contigs_and_models(monkeypatch):
    """A stub in PSMCKernel's place returns known matrices per (model, row): the product sums them over the rows of every contig,
    averages over the models, hands each contig's own length to the kernel, and forms ``expected`` from the row sums and the dense
    transition matrix of each model at per-window rates."""
    import phlash_amd
    from oracle.psmc_numpy import dense_from_pp
    from phlash_amd import decode
    from phlash_amd.kernel import PairCounts
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel

    seen = {}
    rng = np.random.default_rng(0)
    M, ws = 4, 100

    class Stub:
        def __init__(self, M_, rows, double_precision=False, device=None):
            seen["M"], seen["rows"], seen["dbl"] = M_, rows, double_precision
            self.device = torch.device("cpu")

        def pair_counts(self, pp, index, *, lens=None):
            seen["lens"], seen["index"], seen["pp"] = lens, index, pp
            B, N = pp.d.shape[0], len(index)
            seen["mats"] = rng.random((B, N, M, M))
            return PairCounts(torch.zeros(B, N, dtype=torch.float64), torch.as_tensor(seen["mats"]))

    monkeypatch.setattr(decode, "PSMCKernel", Stub)
    dm = DemographicModel.default("4*1", 1e-4, 2e-4)
    dms = [dm, DemographicModel(eta=dm.eta._replace(c=dm.eta.c * 1.5), theta=dm.theta, rho=dm.rho * 2)]
    contigs = [np.zeros((2, 30), dtype=np.int8), np.ones((1, 50), dtype=np.int8)]
    out = phlash_amd.transition_counts(dms, contigs, window_size=ws, double_precision=True)
    assert seen["M"] == M and seen["dbl"] is True and seen["rows"].shape == (3, 50)
    assert (seen["rows"][:2, 30:] == -1).all()  # padded with missing windows ...
    np.testing.assert_array_equal(seen["lens"], [30, 30, 50])  # ... which the kernel masks by each contig's own length
    np.testing.assert_array_equal(seen["index"].numpy(), [0, 1, 2])
    assert seen["pp"].d.shape == (2, 1, M)  # one block per model, broadcast over the rows
    per = seen["mats"].sum(1)
    np.testing.assert_allclose(out.per_model.numpy(), per, rtol=0, atol=1e-14)
    np.testing.assert_allclose(out.counts.numpy(), per.mean(0), rtol=0, atol=1e-14)
    exp = np.zeros((M, M))
    defect = 0.0  # how far the rows of a model's transition matrix are from summing to 1 (PSMCParams: about 1e-9)
    for b, m in enumerate(dms):
        q = PSMCParams.from_dm(DemographicModel(eta=m.eta, theta=float(m.theta) * ws, rho=float(m.rho) * ws))
        np.testing.assert_allclose(seen["pp"].d[b, 0].numpy(), np.asarray(q.d, float), rtol=1e-15)  # per-window rates
        A = dense_from_pp(q)
        defect = max(defect, np.abs(A.sum(1) - 1.0).max())
        exp += per[b].sum(1, keepdims=True) * A / len(dms)
    np.testing.assert_allclose(out.expected.numpy(), exp, rtol=0, atol=1e-13)
    assert defect < 1e-7
    assert abs(float(out.expected.sum()) - float(out.counts.sum())) <= (defect + 1e-14) * float(out.counts.sum())
    assert out.counts.dtype == torch.float64 and out.expected.shape == (M, M)
    # one model, one matrix: the same reduction
    one = phlash_amd.transition_counts(dm, np.zeros((2, 20), dtype=np.int8), window_size=ws)
    assert seen["lens"] is None and one.per_model.shape == (1, M, M)
    np.testing.assert_allclose(one.counts.numpy(), seen["mats"].sum(1)[0], rtol=0, atol=1e-14)
