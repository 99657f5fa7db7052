"""Pair counts on the GPU (phk_pair_counts / PSMCKernel.pair_counts / phlash_amd.transition_counts): the K x K matrix against
the float64 oracle for every compiled K (and a padded one) in both precisions, both parameter layouts, ragged lens, a serial
and a segmented plan; a long float32 row, whose small entries need the float64 partial; the identities that tie the matrix to
phk_transitions and phk_posterior on the same handle; bits under repeats and slabs; a model without recombination; whole
contigs.  Bars: tests/pair_count_bars.py.  The oracle's matrix is asymmetric, so a transposed or permuted accumulator layout
fails the first test.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import pair_count_bars as bars
import pair_count_oracle as pco
from test_pair_counts_cpu import GRID_B, GRID_K, GRID_S, grid_oracle, grid_sets
from test_posterior_decode import _bcast, _pp_np, _population, _rows

pytestmark = pytest.mark.gpu


def _plans(K):
    """a serial and a segmented plan every (K, precision) has kernels for: 4 states per lane in the sweeps"""
    R = max(K // 4, 1)
    Rf = max(R, 2)
    return {"serial": (0, R, 8, Rf, 0), "segmented": (1, R, 16, Rf, Rf)}


@pytest.mark.parametrize("dbl", [False, True])
@pytest.mark.parametrize("K", GRID_K)
def test_pair_counts_against_the_oracle(K, dbl):
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    B, S = GRID_B, GRID_S
    pp = _population(K, B, seed=K)
    pc = _population(K, B * S, seed=1000 + K)
    Kc = 16 if K == 12 else K  # the compiled size (12 is padded to 16)
    worst = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        for layout in ("bcast", "chunk"):
            C, LL = grid_oracle(K)[i, layout]
            q = _bcast(pp) if layout == "bcast" else PSMCParams(*(torch.as_tensor(a).reshape(B, S, K).contiguous() for a in pc))
            for name, plan in _plans(Kc).items():
                kern._eng.set_plan(*plan)
                out = kern.pair_counts(q, np.arange(S), lens=lens)
                c = out.counts.cpu().numpy()
                assert c.shape == C.shape and out.counts.dtype == torch.float64
                assert np.isfinite(c).all() and (c >= 0).all()
                err = pco.error(c, C)
                worst = max(worst, err)
                rel = np.abs(out.ll.cpu().numpy() / LL - 1).max()
                assert rel < (1e-12 if dbl else 1e-5), (name, layout, W, rel)
    print(f"PARITY pair counts K={K} {'f64' if dbl else 'f32'}: max |C - oracle| / max(1, oracle) = {worst:.3e}")
    assert worst < (bars.F64_COUNTS_BAR if dbl else bars.F32_COUNTS_BAR), worst


LONG_L = 40_000


def test_long_row_keeps_its_small_entries():
    """K = 16, float32, one row of 40,000 sites at 1 % hets: an entry is a sum of 40,000 non-negative terms.  A float32
    accumulator carried over the whole row rounds every add to 2^-24 of the running sum; added into a float64 partial every 64
    sites it does not.  Entry-wise over the whole matrix (relative to max(1, oracle)) and, relative to the entry itself, over the
    entries at least 8 states off the diagonal, the small ones.  Measured on the MI355X: see tests/pair_count_bars.py."""
    from phlash_amd.kernel import get_kernel

    rows = _rows(1, LONG_L, seed=40, het=0.01)
    pp = _population(16, 1, seed=41)
    C, ll = pco.pair_counts(_pp_np(pp, 0), rows[0], 0)
    kern = get_kernel(16, rows, double_precision=False, overlap=0)
    i, j = np.indices((16, 16))
    far = np.abs(i - j) >= 8
    assert C[far].max() < 1.0 and C[far].min() > 0.0
    for name, plan in _plans(16).items():
        kern._eng.set_plan(*plan)
        out = kern.pair_counts(_bcast(pp), np.arange(1))
        c = out.counts.cpu().numpy()[0, 0]
        err = pco.error(c, C)
        err_far = float((np.abs(c - C)[far] / C[far]).max())
        print(f"PARITY pair counts long row ({name}): max |C - oracle| / max(1, oracle) = {err:.3e}, "
              f"|i - j| >= 8 relative to the entry = {err_far:.3e} (entries {C[far].min():.2e} .. {C[far].max():.2e})")
        assert abs(float(out.ll[0, 0]) / ll - 1) < 1e-5
        assert err < bars.F32_LONG_ROW_BAR, (name, err)
        assert err_far < bars.F32_LONG_ROW_FAR_REL_BAR, (name, err_far)
        err_t = abs(c.sum() - LONG_L) / LONG_L
        print(f"pair counts long row ({name}): total {err_t:.3e}")
        assert err_t < bars.F32_TOTAL_BAR, (name, err_t)


def _kernel16(dbl=False, S=4, L=5000, W=200, seed=5):
    from phlash_amd.kernel import get_kernel

    rows = _rows(S, L, seed=seed, het=0.05, run=300)
    return rows, get_kernel(16, rows, double_precision=dbl, overlap=W)


@pytest.mark.parametrize("dbl", [False, True])
def test_identities_against_transitions_and_posterior(dbl):
    """On one handle, with ragged lens: the diagonal of counts is the sum over the own sites of phk_transitions' stay (bin = 1),
    its strict-upper column sums that of up and its strict-lower ones that of down; its column sums are the summed marginals of
    phk_posterior; it sums to the number of own scored sites; ll is phk_posterior's to the bit."""
    rows, kern = _kernel16(dbl)
    W, L = kern.overlap, kern.L
    pp = _bcast(_population(16, 3, seed=2))
    inds = np.arange(4)
    lens = np.array([5000, 4321, 201, 777])
    own = torch.as_tensor(np.arange(W, L)[None, :] < lens[:, None], device=kern.device)  # [S, L - W]
    n_own = torch.as_tensor(lens - W, device=kern.device, dtype=torch.float64)
    for name, plan in _plans(16).items():
        kern._eng.set_plan(*plan)
        out = kern.pair_counts(pp, inds, lens=lens)
        c = out.counts
        t = kern.transitions(pp, inds, bin=1, lens=lens)
        arr = (t.arrivals.double() * own[None, :, :, None, None]).sum(2)  # [B, S, 3, K]: bin = 1, own sites in the bin: 1 or 0
        ref = torch.stack([torch.diagonal(c, dim1=-2, dim2=-1), torch.triu(c, 1).sum(-2), torch.tril(c, -1).sum(-2)], -2)
        err_a = float(((ref - arr).abs() / arr.clamp(min=1.0)).max())
        p = kern.posterior(pp, inds, bin=1)
        marg = (p.marginals.double() * own[None, :, :, None]).sum(2)  # [B, S, K]
        err_m = float(((c.sum(-2) - marg).abs() / marg.clamp(min=1.0)).max())
        err_t = float(((c.sum((-1, -2)) - n_own).abs() / n_own).max())
        print(f"pair counts identities ({'f64' if dbl else 'f32'}, {name}): arrivals {err_a:.3e}, marginals {err_m:.3e}, "
              f"total {err_t:.3e}")
        assert torch.equal(out.ll, p.ll) and torch.equal(out.ll, t.ll), name
        assert err_a < (bars.F64_ARRIVALS_IDENTITY_BAR if dbl else bars.F32_ARRIVALS_IDENTITY_BAR), (name, err_a)
        assert err_m < (bars.F64_MARGINALS_IDENTITY_BAR if dbl else bars.F32_MARGINALS_IDENTITY_BAR), (name, err_m)
        assert err_t < (bars.F64_TOTAL_BAR if dbl else bars.F32_TOTAL_BAR), (name, err_t)


def test_bits_under_repeats_slabs_and_beside_a_gradient_call():
    rows, kern = _kernel16(False)
    eng = kern._eng
    pp = _bcast(_population(16, 3, seed=7))
    inds = np.arange(4)
    lens = np.array([5000, 4321, 5000, 777])
    same = lambda x, y: torch.equal(x.counts, y.counts) and torch.equal(x.ll, y.ll)  # noqa: E731
    ll0, g0 = kern(pp, inds, grad=True)  # the gradient call before any pair-count call
    plan0 = eng.get_plan()
    a = kern.pair_counts(pp, inds, lens=lens)
    b = kern.pair_counts(pp, inds, lens=lens)
    assert same(a, b)
    assert eng.get_plan() == plan0
    ll1, g1 = kern(pp, inds, grad=True)
    assert torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert eng.get_plan() == plan0
    res = {}
    for name, plan in _plans(16).items():
        eng.set_plan(*plan)  # (a slab is a launch shape of its own: fix the plan so that both runs use the same one)
        a = kern.pair_counts(pp, inds, lens=lens)
        # 128 KB: 40 KB of checkpoints and 20 KB of partials (10 units) per sequence, so 2 sequences per slab and 6 slabs
        eng.set_workspace_limit(1 << 17)
        c = kern.pair_counts(pp, inds, lens=lens)
        eng.set_workspace_limit(1 << 40)
        assert same(a, c), name
        assert same(a, kern.pair_counts(pp, inds, lens=lens)), name
        res[name] = a.counts
    err = float(((res["serial"] - res["segmented"]).abs() / res["serial"].clamp(min=1.0)).max())
    print(f"pair counts serial vs segmented plan: {err:.3e}")
    assert err < bars.F32_COUNTS_BAR


def test_no_recombination_no_moves():
    """rho about 0 (1e-10 per site; PSMCParams keeps its factors off exact zero): d is about 1, every site stays, and the
    off-diagonal mass of a whole row is below the float32 bar -- in the float64 oracle, which the test checks first, and on the
    GPU, whose off-diagonal mass is the oracle's to the same bar."""
    import phlash_amd
    from phlash_amd.kernel import get_kernel
    from phlash_amd.params import PSMCParams

    rows = _rows(2, 700, seed=9)
    dm = phlash_amd.DemographicModel.default("14*1+1*2", 0.01, 1e-10)
    q = _pp_np(PSMCParams(*(torch.as_tensor(a)[None] for a in PSMCParams.from_dm(dm))), 0)
    ref = [pco.pair_counts(q, rows[s], 0)[0] for s in range(2)]
    ref_mass = max(float(C.sum() - np.trace(C)) for C in ref)
    assert ref_mass < bars.F32_COUNTS_BAR and min(float(np.diag(C).min()) for C in ref) >= 0.0
    kern = get_kernel(16, rows, double_precision=False, overlap=0)
    c = kern.pair_counts(dm, np.arange(2)).counts
    off = c - torch.diag_embed(torch.diagonal(c, dim1=-2, dim2=-1))
    mass = float(off.sum((-1, -2)).max())
    err_t = float((c.sum((-1, -2)) - 700).abs().max()) / 700
    err = max(pco.error(c[s].cpu().numpy(), ref[s]) for s in range(2))
    print(f"pair counts, rho = 1e-10: off-diagonal mass {mass:.3e} (oracle {ref_mass:.3e}), against the oracle {err:.3e}, total {err_t:.3e}")
    assert torch.isfinite(c).all() and mass < bars.F32_COUNTS_BAR
    assert err < bars.F32_COUNTS_BAR
    assert err_t < bars.F32_TOTAL_BAR


def test_transition_counts_on_the_golden_contig(psmcfa_file):
    """The golden .psmcfa contig (one row of 100 windows) and a longer padded one under two models: counts sums to the number
    of windows of the contigs' own, and so does expected, as far as the rows of the models' transition matrices sum to 1 (the
    test measures that defect on the dense float64 matrix and allows it, plus float64 rounding)."""
    import phlash_amd
    from oracle.psmc_numpy import dense_from_pp
    from phlash_amd.data import RawContig
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel

    rc = list(RawContig.from_psmcfa_iter(psmcfa_file, 100))
    assert len(rc) == 1 and rc[0].het_matrix.shape == (1, 100)
    dm = DemographicModel.default("14*1+1*2", 1e-4, 1e-4)
    dms = [dm, DemographicModel(eta=dm.eta._replace(c=dm.eta.c * 1.5), theta=dm.theta, rho=dm.rho)]
    total = 100.0
    out = phlash_amd.transition_counts(dms, rc, window_size=100)
    assert out.counts.shape == (16, 16) and out.per_model.shape == (2, 16, 16) and out.counts.dtype == torch.float64
    defect = 0.0
    for m in dms:
        q = PSMCParams.from_dm(DemographicModel(eta=m.eta, theta=float(m.theta) * 100, rho=float(m.rho) * 100))
        defect = max(defect, float(np.abs(dense_from_pp(q).sum(1) - 1.0).max()))
    cs, es = float(out.counts.sum()), float(out.expected.sum())
    print(f"transition_counts: counts.sum() = {cs!r}, expected.sum() = {es!r}, windows {total}, row-sum defect of A {defect:.2e}")
    assert abs(cs - total) < bars.F32_TOTAL_BAR * total
    assert abs(es - cs) <= (defect + 1e-13) * total
    # a second, shorter contig beside it: padded windows count nothing
    both = phlash_amd.transition_counts(dms, [rc[0], rc[0].het_matrix[:, :37]], window_size=100)
    print(f"transition_counts, two contigs: total {abs(float(both.counts.sum()) - 137.0) / 137:.3e}")
    assert abs(float(both.counts.sum()) - 137.0) < bars.F32_TOTAL_BAR * 137
    assert float((both.per_model.sum((-1, -2)) - 137.0).abs().max()) < bars.F32_TOTAL_BAR * 137
