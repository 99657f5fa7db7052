"""On-demand rescaling of the forward kernels with several states per lane (rescale interval 4): a rescale site only
tests the sum its own scan produced, and a sequence is rescaled once that sum is below 2^-16 (Lane::rescale_on_demand,
DESIGN.md section 2).  The scales are exact powers of two, so against the SAME inputs evaluated with the rescale interval set
to 1 -- the per-site schedule, which the change does not touch -- every gradient row must come back bit for bit and ll to the
last bits of its float64 ``log(c) + E ln 2``; both must also meet the float64 oracle at the bars of tests/parity_bars.py.

Which variants: "bit for bit" compares two evaluations whose sweeps must add the same terms in the same order.  At interval
4 the sweeps with at most 8 float32 / 4 float64 states per lane and T = 8 take the beta-first hot body, which accumulates a
block's sites in ascending order; at interval 1 they take the general body, which accumulates them in descending order: the
same terms, another rounding.  The bitwise cases therefore force sweep variants that run the general body at both intervals
(float32: 16 states per lane; float64: T = 16, or the 8-states-per-lane segment sweep) behind on-demand forward kernels
(R_forward = 1 / 2 / 4); the flagship pair (one-lane forward kernel, two-lane hot-body sweep) is held to the oracle bars and
to the ll agreement in a case of its own.

Inputs: rows of 2,100 / 2,107 sites (past the 2,048-site fold of the partial sums, the second with a partial last block),
W = 37 (warm-up boundary inside a block), 2 % hets + 1 % missing, theta = 0.1: the mass falls by ~0.2 bits per site (CPU:
test_the_chosen_rows_trigger_many_rescales), so the 2^-16 trigger fires 20-odd times per row instead of after every fourth
site."""

import math

import numpy as np
import pytest

from oracle import cport
from oracle import psmc_numpy as o
from parity_bars import F32_GRAD_FULL, F32_GRAD_OWN, F64_GRAD_FULL, F64_GRAD_OWN, grad_error_ratios

THETA = 0.1
TRIGGER_EXP = 16  # PHK_RESCALE_TRIGGER_EXP of psmc_kernels.hip
W = 37
MIN_FIRES = 10


def _params(K, B, seed, model):
    """B particles around the default model at theta = rho = THETA -> [B, 1, 7, K]; "steep": het emissions of 1e-3 everywhere
    (10 bits per het site: a run of eight takes a block past the sweeps' 2^-64 hot-body limit, no group of four reaches the
    2^-64 of the underflow flag -- the model of test_steep_blocks_take_the_general_body)."""
    rng = np.random.default_rng(seed)
    pat = f"{K - 2}*1+1*2"
    x0 = o.particle_from_linear(pat, 1e-4, 15.0, np.ones(len(o.parse_pattern(pat))), THETA, THETA)
    out = np.zeros((B, 1, 7, K))
    for b in range(B):
        x = x0 + 0.3 * rng.normal(size=x0.shape) * (b > 0)
        out[b, 0] = o.from_dm(o.particle_to_dm(x, pat, THETA)).stack()
    if model == "steep":
        out[:, 0, 5] = 1e-3
        out[:, 0, 4] = 1.0 - 1e-3
    return out


def _rows(L, model, n=2):
    rng = np.random.default_rng(L)
    data = (rng.uniform(size=(n, L)) < 0.02).astype(np.int8)
    data[rng.uniform(size=data.shape) < 0.01] = -1
    if model == "steep":
        for r in range(n):
            for s0, m in ((40 + 7 * r, 8), (301, 16), (1100 + r, 9)):
                data[r, s0:s0 + m] = 1
    return data


def _predicted_fires(P7, row, T=8, warmup=W):
    """The schedule of the forward kernel in float64 numpy: full blocks without the warm-up boundary test, after sites 3 and 7
    (11, 15), the sum of the state ENTERING that site against 2^-TRIGGER_EXP; the other blocks rescale after every fourth
    site.  Returns (rescales fired in full blocks, mean log2 of the mass kept per site)."""
    pp = o.PP(*P7)
    a = np.array(pp.pi, dtype=np.float64)
    nfull, blkW = len(row) // T, (warmup - 1) // T if warmup > 0 else -1
    fired, bits = 0, 0.0
    for t, ob in enumerate(row):
        before = a.sum()
        a = o.matvec_smc(a, pp) * o.emission_row(pp, int(ob))
        bits += math.log2(a.sum() / before)
        if t % 4 == 3:
            if t // T < nfull and t // T != blkW:
                if before < 2.0 ** -TRIGGER_EXP:
                    a = a * 2.0 ** -math.frexp(before)[1]
                    fired += 1
            else:
                a = a * 2.0 ** -math.frexp(a.sum())[1]
    return fired, bits / len(row)


@pytest.mark.parametrize("model", ["default", "steep"])
@pytest.mark.parametrize("K,L", [(16, 2100), (16, 2107), (32, 1203), (64, 1203)])
def test_the_chosen_rows_trigger_many_rescales(K, L, model):
    """CPU: theta and the rows are chosen so that the trigger fires many times per row -- and far less often than the fixed
    schedule's twice per block."""
    P, data = _params(K, 3, 11, model), _rows(L, model)
    for b in range(3):
        for row in data:
            fired, bits = _predicted_fires(P[b, 0], row)
            assert MIN_FIRES <= fired <= (L // 8) // 4, (b, fired)
            assert -0.6 < bits < -0.1, bits  # 13 % of the mass per site (default model) ... 27 % (steep, short rows)


# ---- GPU ----------------------------------------------------------------------------------------------------------------

_ORACLE = {}


def _oracle(K, L, model, B):
    """(ll, gradient, W = 0 gradient) of the float64 oracle for B particles x the two rows: computed once per input set and
    shared by every plan and float type (never modified)."""
    key = (K, L, model, B)
    if key not in _ORACLE:
        P, data = _params(K, B, 11, model), _rows(L, model)
        ll, g = cport.batch(P, data, np.arange(2), W)
        _, g_full = cport.batch(P, data, np.arange(2), 0)
        for arr in (ll, g, g_full):
            arr.setflags(write=False)
        _ORACLE[key] = (ll, g, g_full)
    return _ORACLE[key]


# K = 16 plans whose sweeps run the general body at interval 4 AND at interval 1 (see the module docstring)
def _force(eng, plan, dbl, nseq):
    if not dbl:  # one-lane forward kernel (16 states per lane), one-lane sweeps, T = 8
        if plan == "serial":
            eng.set_plan(0, R=1, T=8, R_forward=1, R_scan=0)
        elif plan == "segmented":
            eng.set_plan(1, R=1, T=8, R_forward=1, R_scan=2)
        else:
            eng.install_plan({"segmented": 0, "R": 1, "T": 8, "R_forward": 1, "hybrid_first": nseq // 2, "R_segment_sweep": 1, "R_scan": 2})
    else:  # float64 sweeps own at most 4 states per lane (8 in the segment sweep): T = 16 keeps R = 4 out of the hot body
        if plan == "serial":
            eng.set_plan(0, R=4, T=16, R_forward=4, R_scan=0)
        elif plan == "segmented":
            eng.set_plan(1, R=2, T=8, R_forward=2, R_scan=2)
        else:
            eng.install_plan({"segmented": 0, "R": 4, "T": 16, "R_forward": 4, "hybrid_first": nseq // 2, "R_segment_sweep": 4, "R_scan": 4})


def _evaluate(K, data, P, dbl, force, nrm):
    """(ll, gradient, block-rescale counts, blocks per sequence, underflow flag) of one forced evaluation."""
    import torch
    from phlash_amd.engine import HipEngine

    eng = HipEngine(K, data, double_precision=dbl)
    eng.set_autotune(False)
    force(eng, P.shape[0] * data.shape[0])
    eng.set_rescale_interval(nrm)
    ll, g = eng.run(torch.tensor(P, device="cuda"), torch.arange(data.shape[0], device="cuda"), warmup=W, grad=True)
    torch.cuda.synchronize()
    counts, blocks = eng.block_rescale_counts()
    return ll.cpu().numpy(), g.double().cpu().numpy(), counts, blocks, eng.underflow_risk()


def _meets_the_oracle(ll, g, K, L, model, B, dbl):
    ll_ref, g_ref, g_full = _oracle(K, L, model, B)
    np.testing.assert_allclose(ll, ll_ref, rtol=1e-10 if dbl else 1e-5)
    a, c = (F64_GRAD_OWN, F64_GRAD_FULL) if dbl else (F32_GRAD_OWN, F32_GRAD_FULL)
    r_bound, r_own, r_full = grad_error_ratios(g, g_ref, g_full, _params(K, B, 11, model), a, c)
    print(f"  oracle: ll rel {np.abs(ll / ll_ref - 1).max():.2e}  gradient err / bound {r_bound:.3f} (own {r_own:.2e}, W = 0 row {r_full:.2e})")
    assert r_bound < 1.0, (r_bound, r_own, r_full)


def _on_demand_against_interval_1(K, L, model, dbl, force, bitwise=True):
    data = _rows(L, model)
    out = {}
    for B in (3, 100):
        P = _params(K, B, 11, model)
        ll4, g4, counts, blocks, flag4 = _evaluate(K, data, P, dbl, force, 4)
        ll1, g1, counts1, _, flag1 = _evaluate(K, data, P, dbl, force, 1)
        print(f"K={K} L={L} {model} {'f64' if dbl else 'f32'} B={B}: blocks {blocks}, rescales per sequence {counts.min()}..{counts.max()} "
              f"(interval 1: {counts1.min()}..{counts1.max()}), max |g4 - g1| {np.abs(g4 - g1).max():.3e}, "
              f"ll rel {np.abs(ll4 / ll1 - 1).max():.2e}")
        assert not flag4 and not flag1  # (neither model is extreme: no underflow flag)
        # the trigger fired many times in every sequence, and in few of its blocks
        assert counts.min() >= MIN_FIRES and counts.max() <= blocks // 4, (counts.min(), counts.max(), blocks)
        if bitwise:
            assert np.array_equal(g4, g1), f"gradient differs from the interval-1 evaluation by up to {np.abs(g4 - g1).max():.3e}"
        np.testing.assert_allclose(ll4, ll1, rtol=1e-12, atol=0)
        _meets_the_oracle(ll4, g4, K, L, model, B, dbl)
        _meets_the_oracle(ll1, g1, K, L, model, B, dbl)
        out[B] = g4
    # neighbour independence: what a sequence returns does not depend on the other sequences of its wave
    # (B = 3: one partial wave with idle lane groups; B = 100: waves that straddle the two chunk rows)
    assert np.array_equal(out[100][:3], out[3]), f"B = 100 and B = 3 differ by up to {np.abs(out[100][:3] - out[3]).max():.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["serial", "segmented", "hybrid"])
@pytest.mark.parametrize("model", ["default", "steep"])
@pytest.mark.parametrize("L", [2100, 2107])
@pytest.mark.parametrize("dbl", [False, True])
def test_k16_on_demand_equals_interval_1(dbl, L, model, plan):
    _on_demand_against_interval_1(16, L, model, dbl, lambda eng, nseq: _force(eng, plan, dbl, nseq))


@pytest.mark.gpu
@pytest.mark.parametrize("K,R", [(32, 2), (64, 4)])
def test_other_K_on_demand_equals_interval_1(K, R):
    """K = 32 / 64, float32, 16 states per lane (forward kernel and serial sweep: the general body at both intervals)."""
    _on_demand_against_interval_1(K, 1203, "default", False, lambda eng, nseq: eng.set_plan(0, R=R, T=8, R_forward=R, R_scan=0))


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["default", "steep"])
def test_flagship_pair_meets_the_oracle(model):
    """The pair the headline shape runs: one-lane on-demand forward kernel, two-lane sweep (hot body at interval 4, general
    body at interval 1: not the same order of additions, so no bitwise claim), hybrid plan with the dense beta scan off."""
    _on_demand_against_interval_1(
        16, 2107, model, False, bitwise=False,
        force=lambda eng, nseq: eng.install_plan({"segmented": 0, "R": 2, "T": 8, "R_forward": 1, "hybrid_first": nseq // 2,
                                                  "R_segment_sweep": 2, "R_scan": 2}))


@pytest.mark.gpu
def test_the_underflow_flag_survives():
    """Safety net: het emissions of 1e-11 on a run of het sites take 2^-36 per site -- the sum a rescale site tests is below
    2^-64 three sites on, and the on-demand forward kernel raises the flag as the fixed schedule did."""
    import torch
    from phlash_amd.engine import HipEngine

    P = _params(16, 1, 0, "default")
    P[0, 0, 5] = 1e-11
    P[0, 0, 4] = 1.0 - 1e-11
    data = np.ones((1, 64), dtype=np.int8)
    for dbl, expect in ((False, True), (True, False)):  # float64 is held to 2^-600: safe
        eng = HipEngine(16, data, double_precision=dbl)
        eng.set_autotune(False)
        eng.set_plan(0, R=4 if dbl else 2, T=8, R_forward=2, R_scan=0)
        eng.set_rescale_interval(4)
        assert not eng.underflow_risk()
        eng.run(torch.tensor(P, device="cuda"), torch.arange(1, device="cuda"), warmup=0, grad=True)
        torch.cuda.synchronize()
        assert eng.underflow_risk() == expect
