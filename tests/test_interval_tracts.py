"""Interval tracts (phk_interval_tracts / HipEngine.interval_tracts / PSMCKernel.interval_tracts / phlash_amd.segment_support).

CPU: the float64 oracle against path enumeration, against the likelihood ratio of oracle/psmc_numpy and against the tract
oracle on a regular grid; the structured floor; the ABI's argument check without a device; the host validation, mask packing and
ordering on a stub engine; segment_support's sets and mixture on a stub kernel; the compiler's resource report; the sampling case.
GPU: the log tracts against the oracle for every compiled K (and a padded one) in both precisions with a different list per row;
a tract below the float range; the exact identities (full and empty sets, bits that do not depend on the rest of the call, ll,
gradient calls around it); the identities within tolerance (regular intervals against phk_tracts, plans, the likelihood ratio,
nesting); sampled paths; the public layer; the ABI's refusals and the device-side check of the lists.
"""

from __future__ import annotations

import functools
import glob
import os
import re

import numpy as np
import pytest
import torch

import interval_bars as bars
import interval_oracle as io
import tract_bars
import tract_oracle as to
from test_posterior_decode import _bcast, _pp_np, _population, _random_pp
from test_tracts import GRID_B, GRID_K, GRID_L, GRID_S, SMP_K, SMP_N, SMP_PREFIX, SMP_ROWS, SMP_SEED, SMP_SITES, _chunk, _kernel16, _np, grid_sets, sampled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_TINY_F32 = float(np.log(np.finfo(np.float32).tiny))  # log of the smallest float32 normal


def err_of(x, ref):
    """the tests' metric: |x - ref| / max(1, |ref|), largest"""
    x, ref = np.asarray(x, float), np.asarray(ref, float)
    return float((np.abs(x - ref) / np.maximum(1.0, np.abs(ref))).max()) if ref.size else 0.0


# ------------------------------------------------------------------------------------------------- shared inputs
def _list_a(o):
    """a length-1 interval at position 0, adjacent intervals, intervals across block edges of 8 and 16 sites, one of 150
    positions, one ending at the row's own length o"""
    return [(0, 1), (1, 9), (13, 19), (20, 45), (45, 46), (100, 250), (o - 30, o)]


def _list_b(o):
    return [(3, 4), (5, 30), (30, 62), (64, 72), (o - 1, o)]


def grid_lists(i):
    """the lists of row set i of ``grid_sets()``: a different list per row, one row with an empty list -> (row, start, end) in an
    order that is not the sorted one"""
    _, W, lens = grid_sets()[i]
    own = [int(n) - W for n in lens]
    per_row = [_list_a(own[0]), _list_b(own[1]), []] if i == 0 else [[], _list_a(own[1]), _list_b(own[2])]
    flat = [(s, a, b) for s, lst in enumerate(per_row) for a, b in lst][::-1]
    return tuple(np.array(x, dtype=np.int64) for x in zip(*flat))


def grid_masks(K, n):
    """-> (shared bool [n, K], per-particle bool [B, n, K]): interval j takes a prefix set, an interior set or all but the
    youngest state in turn; the second particle's sets hold one state more"""
    k = np.arange(K)
    kinds = lambda b: [k < (5 * K) // 8 + b, (k >= K // 4) & (k < (3 * K) // 4 + b), k >= 1 - b]  # noqa: E731
    per = np.stack([np.stack([kinds(b)[j % 3] for j in range(n)]) for b in range(GRID_B)])
    return per[0].copy(), per


@functools.lru_cache(maxsize=None)
def grid_oracle(K):
    """-> {(set, layout, mode): (logp [B, n] in the caller's order, ll [B, S])} of the float64 oracle, once per K"""
    pp = _population(K, GRID_B, seed=K)
    pc = _population(K, GRID_B * GRID_S, seed=1000 + K)
    out = {}
    for i, (rows, W, lens) in enumerate(grid_sets()):
        row, start, end = grid_lists(i)
        shared, per = grid_masks(K, len(row))
        for layout in ("bcast", "chunk"):
            for mode in ("shared", "particle"):
                lp = np.empty((GRID_B, len(row)))
                ll = np.empty((GRID_B, GRID_S))
                for b in range(GRID_B):
                    for s in range(GRID_S):
                        q = _pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * GRID_S + s)
                        mine = np.flatnonzero(row == s)
                        sets = shared if mode == "shared" else per[b]
                        lp[b, mine], ll[b, s] = io.dense(q, rows[s], W, [(start[j], end[j], sets[j]) for j in mine])
                lp.setflags(write=False)
                out[i, layout, mode] = (lp, ll)
    return out


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K,L,W", [(2, 8, 0), (3, 7, 1), (4, 6, 0), (4, 6, 1), (3, 8, 1)])
def test_oracle_against_path_enumeration(K, L, W):
    rng = np.random.default_rng(K * 100 + L * 10 + W)
    pp = _random_pp(K, rng)
    data = rng.integers(-1, 2, size=L)
    data[0] = 1
    data[W + 2] = -1  # a missing site inside the second interval
    n = L - W
    length = n - 1  # (a row whose own length is below L: the last interval ends there)
    S = np.arange(K) < max(1, K // 2)
    T = np.arange(K) >= 1
    iv = [(0, 1, S), (1, 3, T), (3, length, S), (length - 1, length, int(0b10)), (0, n, T), (1, 2, np.zeros(K, bool)), (0, 2, np.ones(K, bool))]
    lp, ll = io.dense(pp, data, W, iv)  # a length-1 interval at 0, two adjacent ones, one ending at `length`, a whole row
    lb = io.bruteforce(pp, data, W, iv)
    assert np.isneginf(lp[5]) and np.isneginf(lb[5])
    fin = np.isfinite(lb)
    np.testing.assert_allclose(lp[fin], lb[fin], rtol=0, atol=1e-13)
    assert abs(lp[6]) < 1e-13 and (lp <= 1e-13).all()
    import posterior_oracle as po

    _, llb = po.bruteforce(pp, data, W)
    assert abs(ll - llb) < 1e-12 * abs(llb) + 1e-13


def test_oracle_whole_row_is_a_likelihood_ratio():
    """one interval over a whole row without missing sites: logp = ll(emissions x indicator) - ll of oracle/psmc_numpy"""
    import oracle.psmc_numpy as pn

    rng = np.random.default_rng(3)
    K, L = 8, 120
    pp = _random_pp(K, rng)
    data = (rng.random(L) < 0.1).astype(int)
    ind = ((np.arange(K) >= 1) & (np.arange(K) < 6)).astype(float)
    lp, ll = io.dense(pp, data, 0, [(0, L, ind > 0)])
    ll0 = pn.psmc_ll_dense(pn.dense_from_pp(pp), pp.emis0, pp.emis1, pp.pi, data)
    ll1 = pn.psmc_ll_dense(pn.dense_from_pp(pp), pp.emis0 * ind, pp.emis1 * ind, pp.pi, data)
    assert abs(ll - ll0) < 1e-12 * abs(ll0)
    assert lp[0] < -1 and abs(lp[0] - (ll1 - ll0)) < 1e-12 * abs(ll1 - ll0)


def _regular(own, bin):
    """the whole bins of ``bin`` positions inside a row's own length"""
    return [(k * bin, (k + 1) * bin) for k in range(own // bin)]


def test_oracle_on_a_regular_grid_is_the_log_of_the_tract_oracle():
    K = 8
    pp = _population(K, GRID_B, seed=K)
    k = np.arange(K)
    sets = [k < 5, (k >= 2) & (k < 6)]
    worst = 0.0
    for rows, W, lens in grid_sets():
        for s in range(GRID_S):
            q = _pp_np(pp, s % GRID_B)
            for bin in (7, 100):
                iv = _regular(int(lens[s]) - W, bin)
                t, ll_t = to.dense(q, rows[s], np.stack(sets).astype(float), W, bin, int(lens[s]))
                for j, S in enumerate(sets):
                    lp, ll = io.dense(q, rows[s], W, [(a, b, S) for a, b in iv])
                    worst = max(worst, err_of(lp, np.log(t[j][: len(iv)])))
                    assert abs(ll - ll_t) < 1e-11 * abs(ll)
    print(f"interval oracle vs log(tract oracle) on regular grids: {worst:.3e}")
    assert worst < 1e-11


@functools.lru_cache(maxsize=None)
def structured_floor(K):
    """log of the structured float64 statement of the kernel's recursion (tract_oracle.structured) against the interval oracle on
    regular intervals of 7 and 100 positions of the grid's rows, both layouts, a prefix and an interior set, in the tests' metric"""
    pp = _population(K, GRID_B, seed=K)
    pc = _population(K, GRID_B * GRID_S, seed=1000 + K)
    shared, _ = grid_masks(K, 2)
    worst = 0.0
    for rows, W, lens in grid_sets():
        for layout in ("bcast", "chunk"):
            for b in range(GRID_B):
                for s in range(GRID_S):
                    q = _pp_np(pp, b) if layout == "bcast" else _pp_np(pc, b * GRID_S + s)
                    tr = to.structured(q, rows[s], shared.astype(float), W, (7, 100), int(lens[s]))
                    for bin, t in zip((7, 100), tr):
                        iv = _regular(int(lens[s]) - W, bin)
                        for j in range(2):
                            lp, _ = io.dense(q, rows[s], W, [(a, c, shared[j]) for a, c in iv])
                            worst = max(worst, err_of(np.log(t[j][: len(iv)]), lp))
    return worst


@pytest.mark.parametrize("K", GRID_K)
def test_structured_floor(K):
    worst = structured_floor(K)
    print(f"PARITY interval tracts structured-vs-oracle K={K}: {worst:.3e}")
    assert worst < bars.STRUCTURED_FLOOR_BAR, worst


def test_bars_are_within_their_caps():
    assert bars.F32_GRID_BAR <= 1e-5
    assert bars.F64_GRID_BAR <= 10 * bars.STRUCTURED_FLOOR


def test_phk_interval_tracts_rejects_a_null_handle_without_a_device():
    from phlash_amd import _lib

    lib = _lib.load()
    assert "phk_interval_tracts" in _lib.SIGNATURES and len(_lib.SIGNATURES["phk_interval_tracts"][1]) == 19
    # (on a thread of its own: the library's last-error string is per thread, and test_layout, which runs later in this
    # process, expects the main thread's to be empty still)
    import threading

    got = []

    def call():
        rc = lib.phk_interval_tracts(None, None, 0, 0, None, None, 1, 1, 0, 1, None, None, None, None, None, 0, None, None, None)
        got.append((rc, lib.phk_last_error()))

    t = threading.Thread(target=call)
    t.start()
    t.join()
    assert got[0][0] == _lib.PHK_EINVAL
    assert b"handle is NULL" in got[0][1]


class _StubEngine:
    """in HipEngine's place: records what PSMCKernel.interval_tracts hands over, returns logp = the sorted position"""

    def __init__(self):
        self.calls = []

    def interval_tracts(self, pa, inds, off, start, end, masks, warmup, max_len, lens):
        self.calls.append(dict(off=off.numpy().copy(), start=start.numpy().copy(), end=end.numpy().copy(), masks=masks.numpy().copy(),
                               warmup=warmup, max_len=max_len))
        B, n = pa.shape[0], start.shape[0]
        return torch.zeros(B, inds.shape[0], dtype=torch.float64), torch.arange(n, dtype=torch.float64).repeat(B, 1) + 100.0 * torch.arange(B)[:, None]

    def underflow_risk(self):
        return False


def _stub_kernel(M=4, N=3, L=50, W=5):
    from phlash_amd.kernel import PSMCKernel

    kern = object.__new__(PSMCKernel)
    kern.M, kern.N, kern.L, kern.overlap, kern.double_precision = M, N, L, W, False
    kern.device = torch.device("cpu")
    kern._eng = _StubEngine()
    return kern


def _stub_pp(M, B):
    from phlash_amd.params import PSMCParams

    return PSMCParams(*(torch.full((B, 1, M), 0.1, dtype=torch.float64) for _ in PSMCParams._fields))


def test_host_validation_ordering_and_masks_on_a_stub_engine():
    kern = _stub_kernel()
    pp = _stub_pp(4, 2)
    inds = np.arange(3)
    lens = np.array([50, 30, 50])
    # the caller's order is not the sorted one: rows 2, 0, 0, 1; the sorted order is entries 2, 1, 3, 0
    iv = (np.array([2, 0, 0, 1]), np.array([0, 10, 3, 20]), np.array([45, 12, 10, 25]))
    masks = np.array([0b0001, 0b0110, 0b1111, 0b1000])
    out = kern.interval_tracts(pp, inds, intervals=iv, masks=masks, lens=lens)
    c = kern._eng.calls[-1]
    assert c["off"].tolist() == [0, 2, 3, 4] and c["start"].tolist() == [3, 10, 20, 0] and c["end"].tolist() == [10, 12, 25, 45]
    assert c["masks"].tolist() == [0b1111, 0b0110, 0b1000, 0b0001] and c["max_len"] == 45 and c["warmup"] == 5
    assert out.logp.shape == (2, 4) and out.logp[0].tolist() == [3.0, 1.0, 0.0, 2.0] and out.logp[1].tolist() == [103.0, 101.0, 100.0, 102.0]
    # tensors as tmrca_segments returns them (a fourth entry is ignored), one model: logp [n]
    one = kern.interval_tracts(_stub_pp(4, 1), 1, intervals=tuple(torch.tensor(x) for x in ([0, 0], [5, 0], [9, 5], [1, 2])),
                               masks=np.array([[True, False, True, False], [False, False, False, True]]))
    assert one.logp.shape == (1, 2) or one.logp.shape == (2,)
    assert kern._eng.calls[-1]["masks"].tolist() == [0b1000, 0b0101]
    # per-particle boolean rows
    per = np.zeros((2, 4, 4), bool)
    per[0, :, 0] = per[1, :, 3] = True
    kern.interval_tracts(pp, inds, intervals=iv, masks=per)
    assert kern._eng.calls[-1]["masks"].tolist() == [[1] * 4, [8] * 4]
    # every bad list is refused on the host, with the offending entry
    bad = {
        "overlaps": (np.array([0, 0]), np.array([0, 4]), np.array([5, 9])),
        "empty": (np.array([0, 0]), np.array([0, 7]), np.array([5, 7])),
        "start below 0": (np.array([0]), np.array([-1]), np.array([5])),
        "beyond the row's own length": (np.array([0, 1]), np.array([0, 20]), np.array([5, 26])),  # lens[1] - W = 25
        "row outside": (np.array([3]), np.array([0]), np.array([5])),
    }
    n_before = len(kern._eng.calls)
    for what, ivb in bad.items():
        with pytest.raises(ValueError, match=what) as e:
            kern.interval_tracts(pp, inds, intervals=ivb, masks=np.zeros(len(ivb[0]), dtype=np.int64), lens=lens)
        assert f"interval {len(ivb[0]) - 1} " in str(e.value)
    with pytest.raises(ValueError, match="beyond"):
        kern.interval_tracts(pp, inds, intervals=(np.array([0]), np.array([40]), np.array([46])), masks=np.array([1]))  # L - W = 45
    assert len(kern._eng.calls) == n_before
    # adjacent intervals and one ending at the row's own length are fine
    kern.interval_tracts(pp, inds, intervals=(np.array([1, 1]), np.array([0, 5]), np.array([5, 25])), masks=np.array([1, 1]), lens=lens)


def test_mask_packing_with_a_padded_K():
    from phlash_amd.kernel import pack_state_masks

    rows = np.zeros((3, 12), bool)
    rows[0, [0, 11]] = True
    rows[1, :] = True
    w = pack_state_masks(rows, 3, 2, 12)
    assert w.dtype == np.uint64 and w.tolist() == [1 | 1 << 11, (1 << 12) - 1, 0]
    # integer masks: bits at or above the model's state count are dropped; a negative int64 is its bit pattern
    assert pack_state_masks(np.array([-1, 1 << 12, 5]), 3, 2, 12).tolist() == [(1 << 12) - 1, 0, 5]
    assert pack_state_masks(np.array([-1], dtype=np.int64), 1, 1, 64).tolist() == [(1 << 64) - 1]
    full = np.ones((1, 64), bool)
    assert pack_state_masks(full, 1, 1, 64).tolist() == [(1 << 64) - 1]
    assert pack_state_masks(torch.tensor([[3, 4], [1, 2]]), 2, 2, 4).tolist() == [[3, 4], [1, 2]]


def test_segment_support_sets_and_mixture_on_a_stub_kernel(monkeypatch):
    import phlash_amd
    from phlash_amd import decode

    assert phlash_amd.segment_support is decode.segment_support and phlash_amd.SegmentSupport is decode.SegmentSupport
    seen = {}

    class Stub:
        def __init__(self, M, rows, double_precision=False, device=None):
            self.M, self.device, self.rows = M, torch.device("cpu"), rows

        def tracts(self, pp, index, *, weights, bin, lens):
            seen["weights"] = np.asarray(weights)
            return Tracts(None, torch.zeros(weights.shape[0], self.rows.shape[0], 5))

        def interval_tracts(self, pp, index, *, intervals, masks, lens):
            seen.update(intervals=intervals, masks=np.asarray(masks), lens=lens)
            B, n = pp.d.shape[0], len(intervals[0])
            return IntervalTracts(None, -torch.arange(1, B * n + 1, dtype=torch.float64).reshape(B, n))

    from phlash_amd.kernel import IntervalTracts, Tracts

    monkeypatch.setattr(decode, "PSMCKernel", Stub)
    M = 8
    dm = phlash_amd.DemographicModel.default(f"{M}*1", 1e-4, 1e-4)
    dm2 = phlash_amd.DemographicModel(eta=dm.eta._replace(t=dm.eta.t * 1.7), theta=dm.theta, rho=dm.rho)
    data = np.zeros((2, 40), dtype=np.int8)
    seg = (torch.tensor([0, 0, 1]), torch.tensor([0, 10, 5]), torch.tensor([10, 30, 40]), torch.tensor([0, 3, 7]))
    # a time range: per model, tract_posterior's weight rows, the same for every segment
    t_min, t_max = float(dm.eta.t[1]), float(dm.eta.t[5])
    decode.tract_posterior([dm, dm2], data, t_max, t_min=t_min, bin=8)
    out = decode.segment_support([dm, dm2], data, seg, t_max=t_max, t_min=t_min)
    assert seen["masks"].shape == (2, 3, M) and seen["masks"].dtype == bool
    for j in range(3):
        assert np.array_equal(seen["masks"][:, j, :].astype(float), seen["weights"])
    assert seen["weights"][0].any() and not np.array_equal(seen["weights"][0], seen["weights"][1])
    # states / slack: the states within slack of the segment's own, as an indicator row per segment
    out = decode.segment_support([dm, dm2], data, seg, slack=1)
    k = np.arange(M)
    assert np.array_equal(seen["masks"], np.stack([np.abs(k - s) <= 1 for s in (0, 3, 7)]))
    decode.segment_support(dm, data, seg[:3], states=[1, 1, 2], slack=0)
    assert np.array_equal(seen["masks"], np.stack([k == s for s in (1, 1, 2)]))
    # the mixture: logsumexp over the models - log B
    assert out.per_model.shape == (2, 3) and out.per_model.dtype == torch.float64
    want = np.log(np.exp(out.per_model.numpy()).mean(0))
    assert np.abs(out.logp.numpy() - want).max() < 1e-12
    # contigs of different lengths: rows are counted per contig, each row's own length goes to the kernel
    res = decode.segment_support(dm, [data[:1, :25], data], [(np.array([0]), np.array([3]), np.array([25]), np.array([2])), seg])
    assert seen["intervals"][0].tolist() == [0, 1, 1, 2] and seen["lens"].tolist() == [25, 40, 40]
    assert [tuple(x.shape) for x in res.logp] == [(1,), (3,)] and [tuple(x.shape) for x in res.per_model] == [(1, 1), (1, 3)]


def _resources(stem):
    """{(real, K): [(kernel, scratch bytes, waves per SIMD)]} from the build's resource reports of launch_<stem>_*"""
    out = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "phlash_amd", "csrc", "build", f"launch_{stem}_f*.o.log"))):
        real, K = re.search(rf"launch_{stem}_(f\d+)_(\d+)\.o\.log$", f).groups()
        rows, cur = [], None
        for line in open(f):
            m = re.search(r"remark:\s+([^:]+): (.+?) \[-Rpass", line)
            if not m:
                continue
            key, val = m.group(1).strip(), m.group(2).strip()
            if key == "Function Name":
                cur = {"name": val}
                rows.append(cur)
            elif cur is not None:
                cur[key] = val
        out[real, int(K)] = [(r["name"], int(r["ScratchSize [bytes/lane]"]), int(r["Occupancy [waves/SIMD]"])) for r in rows if "_kernel" in r["name"]]
    return out


def test_interval_objects_keep_the_tract_objects_resources():
    """The K = 16 float32 object keeps two waves per SIMD, and no interval object uses scratch where the tract object of the same
    (type, K) uses none."""
    iv, tr = _resources("interval"), _resources("tract")
    if len(tr) < 10:
        pytest.skip("no build logs (the library was not built in this tree)")
    assert sorted(iv) == sorted(tr) and len(iv) == 10
    assert all("interval_kernel" in n for rows in iv.values() for n, _, _ in rows)
    assert len(iv["f32", 16]) == 12 and min(occ for _, _, occ in iv["f32", 16]) >= 2  # (T, NRM, SEG) = 2 x 3 x 2 kernels
    for key, rows in iv.items():
        if not any(s for _, s, _ in tr[key]):
            assert not [(n, s) for n, s, _ in rows if s], (key, [(n, s) for n, s, _ in rows if s])


SMP_LEN = 50


def sampling_intervals():
    """24 intervals of 50 windows at offsets that are no multiples of 50, over four chunk positions (the two rows of ``sampled()``,
    twice): 11 adjacent ones from position 13 on the first two, one at 531 on the other two"""
    pos = [(s, 13 + SMP_LEN * k) for s in (0, 1) for k in range(11)] + [(2, 531), (3, 531)]
    row, start = np.array(pos).T
    return row, start, start + SMP_LEN


@functools.lru_cache(maxsize=None)
def sampling_oracle():
    from phlash_amd.params import PSMCParams

    data, dm, m, _ = sampled()
    q = _pp_np(PSMCParams(*(torch.as_tensor(a)[None] for a in PSMCParams.from_dm(dm))), 0)
    row, start, end = sampling_intervals()
    lp = np.empty(len(row))
    for s in range(4):
        mine = np.flatnonzero(row == s)
        lp[mine], _ = io.dense(q, data[s % SMP_ROWS], 0, [(start[j], end[j], m > 0) for j in mine])
    return lp


def test_sampling_case_has_enough_intervals():
    row, start, end = sampling_intervals()
    p = np.exp(sampling_oracle())
    ok = SMP_N * p * (1 - p) >= 25
    print(f"path-sampling case: oracle probabilities {np.round(p, 4).tolist()}, {int(ok.sum())} of {p.size} intervals qualify")
    assert p.size == 24 and (start % SMP_LEN != 0).all() and (end <= SMP_SITES).all()
    assert ok.sum() >= 8


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
@pytest.mark.parametrize("K", GRID_K)
def test_intervals_against_the_oracle(K, dbl):
    from phlash_amd.kernel import get_kernel

    B, S = GRID_B, GRID_S
    pp = _population(K, B, seed=K)
    pc = _population(K, B * S, seed=1000 + K)
    worst = 0.0
    for i, (rows, W, lens) in enumerate(grid_sets()):
        kern = get_kernel(K, rows, double_precision=dbl, overlap=W)
        iv = grid_lists(i)
        shared, per = grid_masks(K, len(iv[0]))
        for layout in ("bcast", "chunk"):
            q = _bcast(pp) if layout == "bcast" else _chunk(pc, B, S, K)
            for mode, masks in (("shared", shared), ("particle", per)):
                ref, LL = grid_oracle(K)[i, layout, mode]
                out = kern.interval_tracts(q, np.arange(S), intervals=iv, masks=masks, lens=lens)
                lp = out.logp.cpu().numpy()
                assert lp.shape == ref.shape and lp.dtype == np.float64
                assert np.isfinite(lp).all() and (lp <= 0).all() and np.isfinite(ref).all()
                e = err_of(lp, ref)
                print(f"interval tracts K={K} {'f64' if dbl else 'f32'} set {i} {layout} {mode}: {e:.3e} (logp {ref.min():.1f} .. {ref.max():.3f})")
                worst = max(worst, e)
                rel = np.abs(out.ll.cpu().numpy() / LL - 1).max()
                assert rel < (1e-12 if dbl else 1e-5), (layout, W, rel)
    print(f"PARITY interval tracts K={K} {'f64' if dbl else 'f32'}: max |logp - oracle| / max(1, |oracle|) = {worst:.3e}")
    assert worst < (bars.F64_GRID_BAR if dbl else bars.F32_GRID_BAR), worst


LONG_SET = (np.arange(16) >= 4) & (np.arange(16) < 12)  # a narrow interior set


@pytest.mark.gpu
def test_a_tract_below_the_float_range_is_right_as_a_log():
    """float32, K = 16: one interval of 4,000 windows of a 5,000-window row whose probability is below the smallest float32
    normal.  phk_tracts keeps q on beta's scale and returns 0 there; the log with its own exponent is finite and right."""
    rows, kern = _kernel16(False)
    q = _population(16, 1, seed=2)
    S, n = rows.shape[0], 4000
    iv = (np.arange(S), np.zeros(S, dtype=np.int64), np.full(S, n))
    ref = np.array([io.dense(_pp_np(q, 0), rows[s], kern.overlap, [(0, n, LONG_SET)])[0][0] for s in range(S)])
    assert (ref < LOG_TINY_F32).all(), ref
    out = kern.interval_tracts(_bcast(q), np.arange(S), intervals=iv, masks=np.tile(LONG_SET, (S, 1)))
    lp = out.logp.cpu().numpy()[0]
    with np.errstate(divide="ignore"):
        lin = np.log(_np(kern.tracts(_bcast(q), np.arange(S), weights=LONG_SET.astype(float), bin=n).prob)[0, :, 0])
    e = err_of(lp, ref)
    print(f"oracle logp {ref.tolist()}\nkernel logp {lp.tolist()}\nlog(phk_tracts at bin = {n}) {lin.tolist()}")
    print(f"per-window error {(np.abs(lp - ref) / n).max():.3e}")
    print(f"PARITY interval tracts 4,000-window interval f32: |logp - oracle| / max(1, |oracle|) = {e:.3e}")
    assert np.isfinite(lp).all()
    assert e < bars.F32_LONG_BAR, e


def _lists16():
    """lists of the _kernel16 rows (W = 200, own lengths 4800, 4121, 4800, 577): an interval of 600 windows, longer than a
    512-site segment; last sites on the first (512) and on the last (1023) site of a unit of the segmented plan; adjacent
    intervals; a row with an empty list"""
    per_row = [[(300, 313), (313, 400), (700, 824), (900, 1500), (4700, 4800)], [(0, 1), (100, 700), (824, 830), (4100, 4121)], [], [(10, 500)]]
    flat = [(s, a, b) for s, lst in enumerate(per_row) for a, b in lst]
    return tuple(np.array(x, dtype=np.int64) for x in zip(*flat))


LENS16 = np.array([5000, 4321, 5000, 777])


def _masks16(n, B=3):
    k = np.arange(16)
    return np.stack([np.stack([(k < 8 + b) if j % 2 == 0 else (k >= 2) & (k < 11 + b) for j in range(n)]) for b in range(B)])


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_full_and_empty_sets_are_exact(dbl):
    rows, kern = _kernel16(dbl)
    pp = _bcast(_population(16, 3, seed=2))
    iv = _lists16()
    n = len(iv[0])
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        kern._eng.set_plan(*plan)
        full = kern.interval_tracts(pp, np.arange(4), intervals=iv, masks=np.full(n, (1 << 16) - 1), lens=LENS16).logp
        assert bool((full == 0.0).all()), full
        none = kern.interval_tracts(pp, np.arange(4), intervals=iv, masks=np.zeros(n, dtype=np.int64), lens=LENS16).logp
        assert bool(torch.isneginf(none).all()), none
    # a padded K: the bits of the model's own states are the full set
    rows12, W, lens = grid_sets()[1]
    kern = __import__("phlash_amd.kernel", fromlist=["get_kernel"]).get_kernel(12, rows12, double_precision=dbl, overlap=W)
    iv = grid_lists(1)
    full = kern.interval_tracts(_bcast(_population(12, 2, seed=12)), np.arange(3), intervals=iv, masks=np.ones((len(iv[0]), 12), bool), lens=lens).logp
    assert bool((full == 0.0).all()), full


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_rest_of_the_call():
    rows, kern = _kernel16(False)
    eng = kern._eng
    pp = _bcast(_population(16, 3, seed=7))
    inds = np.arange(4)
    iv = _lists16()
    n = len(iv[0])
    masks = _masks16(n)
    ll0, g0 = kern(pp, inds, grad=True)  # the gradient call before any interval call
    plan0 = eng.get_plan()
    a = kern.interval_tracts(pp, inds, intervals=iv, masks=masks, lens=LENS16)
    b = kern.interval_tracts(pp, inds, intervals=iv, masks=masks, lens=LENS16)
    assert torch.equal(a.logp, b.logp) and torch.equal(a.ll, b.ll)
    ll1, g1 = kern(pp, inds, grad=True)
    assert torch.equal(ll0, ll1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert eng.get_plan() == plan0
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        eng.set_plan(*plan)
        a = kern.interval_tracts(pp, inds, intervals=iv, masks=masks, lens=LENS16)
        assert a.logp.shape == (3, n) and bool(torch.isfinite(a.logp).all())
        # every interval alone in the call's list
        for j in range(n):
            one = kern.interval_tracts(pp, inds, intervals=tuple(x[j : j + 1] for x in iv), masks=masks[:, j : j + 1], lens=LENS16)
            assert torch.equal(one.logp[:, 0], a.logp[:, j]), (plan, j)
        # the other rows' lists change: row 0's intervals with nothing else, and with another list on rows 2 and 3
        mine = np.flatnonzero(iv[0] == 0)
        other = (np.array([2, 3, 3]), np.array([5, 0, 40]), np.array([4000, 40, 41]))
        both = tuple(np.concatenate([x[mine], y]) for x, y in zip(iv, other))
        mb = np.concatenate([masks[:, mine], masks[:, :3]], axis=1)
        c = kern.interval_tracts(pp, inds, intervals=both, masks=mb, lens=LENS16)
        assert torch.equal(c.logp[:, : len(mine)], a.logp[:, mine]), plan
        # slabs: three sequences per launch
        eng.set_workspace_limit(1 << 17)
        d = kern.interval_tracts(pp, inds, intervals=iv, masks=masks, lens=LENS16)
        eng.set_workspace_limit(1 << 40)
        assert torch.equal(d.logp, a.logp) and torch.equal(d.ll, a.ll), plan
        # ll is phk_posterior's, to the bit
        assert torch.equal(a.ll, kern.posterior(pp, inds, bin=7).ll), plan


@pytest.mark.gpu
def test_plans_agree_and_a_sub_interval_is_no_less_probable():
    rows, kern = _kernel16(False)
    eng = kern._eng
    pp = _bcast(_population(16, 3, seed=7))
    inds = np.arange(4)
    iv = _lists16()
    masks = _masks16(len(iv[0]))
    kern(pp, inds, grad=True)  # (get_plan reports the plan of the last gradient call's shape)
    eng.set_plan(0, 4, 8, 4, 0)
    ser = kern.interval_tracts(pp, inds, intervals=iv, masks=masks, lens=LENS16).logp.cpu().numpy()
    eng.set_plan(1, 4, 16, 4, 4)
    assert eng.get_plan()["segmented"] == 1
    seg = kern.interval_tracts(pp, inds, intervals=iv, masks=masks, lens=LENS16).logp.cpu().numpy()
    e = err_of(seg, ser)
    print(f"serial vs segmented plan: {e:.3e} (logp {ser.min():.1f} .. {ser.max():.3f})")
    assert e < bars.F32_GRID_BAR
    # sub-intervals of (900, 1500) on row 0 and of (100, 700) on row 1, the same set: at least the container's logp
    k = np.arange(16)
    S = (k >= 2) & (k < 11)
    outer = (np.array([0, 1]), np.array([900, 100]), np.array([1500, 700]))
    inner = (np.array([0, 0, 1, 1]), np.array([900, 1200, 100, 699]), np.array([1100, 1500, 101, 700]))
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        eng.set_plan(*plan)
        lo = kern.interval_tracts(pp, inds, intervals=outer, masks=np.tile(S, (2, 1)), lens=LENS16).logp.cpu().numpy()
        li = kern.interval_tracts(pp, inds, intervals=inner, masks=np.tile(S, (4, 1)), lens=LENS16).logp.cpu().numpy()
        cont = lo[:, [0, 0, 1, 1]]
        print(f"plan {plan}: min (sub-interval - container) / max(1, |container|) = {((li - cont) / np.maximum(1, np.abs(cont))).min():.3e}")
        assert (li >= cont - bars.F32_GRID_BAR * np.maximum(1, np.abs(cont))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dbl", [False, True])
def test_regular_intervals_are_the_log_of_phk_tracts(dbl):
    rows, kern = _kernel16(dbl)
    pp = _bcast(_population(16, 3, seed=2))
    inds = np.arange(4)
    k = np.arange(16)
    w = np.stack([(k < 8 + b) for b in range(3)])
    own = LENS16 - kern.overlap
    for bin in (7, 100):
        lists = [(s, a, b) for s in range(4) for a, b in _regular(int(own[s]), bin)]
        iv = tuple(np.array(x) for x in zip(*lists))
        lp = kern.interval_tracts(pp, inds, intervals=iv, masks=np.repeat(w[:, None, :], len(lists), axis=1), lens=LENS16).logp.cpu().numpy()
        t = _np(kern.tracts(pp, inds, weights=w.astype(float), bin=bin, lens=LENS16).prob)  # [B, S, nbin]
        ref = np.log(t[:, iv[0], iv[1] // bin])
        # the tract bar is an absolute error of the probability: as an error of its log it is bar / p
        tb = (tract_bars.F64_TRACT_BAR if dbl else tract_bars.F32_TRACT_BAR) / np.exp(ref)
        tol = (bars.F64_GRID_BAR if dbl else bars.F32_GRID_BAR) * np.maximum(1, np.abs(ref)) + tb
        print(f"regular intervals of {bin} vs log(phk_tracts) ({'f64' if dbl else 'f32'}): max |diff| {np.abs(lp - ref).max():.3e}, "
              f"largest share of the tolerance {(np.abs(lp - ref) / tol).max():.3f}")
        assert (np.abs(lp - ref) <= tol).all()


@pytest.mark.gpu
def test_a_whole_row_is_the_likelihood_ratio_of_loglik():
    """One interval over a whole row, W = 0, no missing sites, float64, K = 16: logp = ll(emis0, emis1 multiplied by the indicator)
    - ll, both from the shipped no-gradient call."""
    from phlash_amd.kernel import get_kernel

    L = 200
    rng = np.random.default_rng(17)
    data = (rng.random((2, L)) < 0.05).astype(np.int8)
    data[:, 0] = 1
    kern = get_kernel(16, data, double_precision=True, overlap=0)
    q = _population(16, 2, seed=4)
    k = np.arange(16)
    m = np.stack([(k >= 1) & (k < 12 + b) for b in range(2)])
    out = kern.interval_tracts(_bcast(q), np.arange(2), intervals=(np.arange(2), np.zeros(2, int), np.full(2, L)), masks=np.repeat(m[:, None, :], 2, axis=1))
    lp = out.logp.cpu().numpy()
    mt = torch.as_tensor(m.astype(float))
    qm = q._replace(emis0=torch.as_tensor(q.emis0) * mt, emis1=torch.as_tensor(q.emis1) * mt)
    ll0 = np.asarray(kern(_bcast(q), np.arange(2), grad=False).cpu().numpy(), float)
    ll1 = np.asarray(kern(_bcast(qm), np.arange(2), grad=False).cpu().numpy(), float)
    err = np.abs(lp - (ll1 - ll0)).max()
    print(f"logp {lp.tolist()}, ll ratio {(ll1 - ll0).tolist()}")
    print(f"PARITY interval tracts likelihood-ratio identity: max |logp - (ll_m - ll)| = {err:.3e}")
    assert (lp < -1).all()
    assert err < tract_bars.F64_LIKELIHOOD_RATIO_BAR, err


@pytest.mark.gpu
def test_sampled_paths_stay_in_the_set_as_often_as_logp_says():
    """K = 16 float32, 4,000 draws, 24 intervals of 50 windows off the grid of 50: for every interval with n p (1 - p) >= 25 (p the
    oracle's), |share of draws that stay inside - exp(logp)| <= 5 sqrt(p (1 - p) / n)."""
    from phlash_amd.kernel import get_kernel

    data, dm, m, _ = sampled()
    kern = get_kernel(SMP_K, data, double_precision=False)
    row, start, end = sampling_intervals()
    p = np.exp(sampling_oracle())
    lp = kern.interval_tracts(dm, np.array([0, 1, 0, 1]), intervals=(row, start, end), masks=np.tile(m > 0, (len(row), 1))).logp.cpu().numpy()
    assert lp.shape == (24,)
    paths = kern.sample_paths(dm, np.arange(SMP_ROWS), n_samples=SMP_N, seed=SMP_SEED).paths  # [rows, n, L]
    inside = torch.as_tensor(m > 0, device=paths.device)[paths.long()]
    share = np.array([float(inside[r % SMP_ROWS, :, a:b].all(-1).double().mean()) for r, a, b in zip(row, start, end)])
    ok = SMP_N * p * (1 - p) >= 25
    assert ok.sum() >= 8
    z = np.abs(share - np.exp(lp)) / np.sqrt(p * (1 - p) / SMP_N)
    print(f"qualifying intervals {int(ok.sum())} of {p.size}; exp(logp) {np.round(np.exp(lp[ok]), 4).tolist()}; share of draws "
          f"{np.round(share[ok], 4).tolist()}; worst |share - exp(logp)| in standard errors {z[ok].max():.2f}")
    assert err_of(lp, np.log(p)) < bars.F32_GRID_BAR
    assert (z[ok] <= 5).all(), z[ok]


@pytest.mark.gpu
def test_segment_support_of_viterbi_segments():
    import phlash_amd
    from phlash_amd.kernel import PSMCKernel
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel

    data, dm, _, _ = sampled()
    ws = 100
    dms = [DemographicModel(eta=dm.eta, theta=dm.theta / ws, rho=dm.rho / ws),
           DemographicModel(eta=dm.eta._replace(c=dm.eta.c * 1.5), theta=dm.theta / ws, rho=dm.rho / ws)]
    contigs = [data[:1, :345], data[1:, :]]
    paths, _ = phlash_amd.viterbi_tmrca(dms[0], contigs, window_size=ws)
    tables = [phlash_amd.tmrca_segments(p) for p in paths]
    assert all(len(t[0]) >= 1 for t in tables), [len(t[0]) for t in tables]
    rag = phlash_amd.segment_support(dms[0], contigs, tables, window_size=ws)
    assert [tuple(x.shape) for x in rag.logp] == [(len(t[0]),) for t in tables]

    def pieces(t, n=60):
        """the table with every segment cut into pieces of at most n windows (the most probable path of these rows has few segments)"""
        out = [(int(r), a, min(a + n, int(e)), int(z)) for r, s, e, z in zip(*(x.tolist() for x in t)) for a in range(int(s), int(e), n)]
        return tuple(torch.tensor(x) for x in zip(*out))

    tables = [pieces(t) for t in tables]
    assert sum(len(t[0]) for t in tables) >= 15
    rag = phlash_amd.segment_support(dms[0], contigs, tables, window_size=ws)
    for c, t, lp, pm in zip(contigs, tables, rag.logp, rag.per_model):
        alone = phlash_amd.segment_support(dms[0], c, t, window_size=ws)
        assert lp.shape == (len(t[0]),) and pm.shape == (1, len(t[0])) and lp.dtype == torch.float64
        e = err_of(lp.cpu().numpy(), alone.logp.cpu().numpy())
        print(f"contig of {c.shape[1]} windows, {len(t[0])} segments, padded vs alone: {e:.3e}; logp {float(lp.min()):.2f} .. {float(lp.max()):.3f}")
        assert e < bars.F32_GRID_BAR and bool((lp <= 0).all()) and bool(torch.isfinite(lp).all())
    # states / slack against explicit masks, bitwise
    t = phlash_amd.tmrca_segments(phlash_amd.viterbi_tmrca(dms[0], data, window_size=ws)[0])
    t = pieces(t)
    sup = phlash_amd.segment_support(dms[0], data, t, slack=2, window_size=ws)
    kern = PSMCKernel(SMP_K, data)
    per = DemographicModel(eta=dm.eta, theta=float(dms[0].theta) * ws, rho=float(dms[0].rho) * ws)
    pp = PSMCParams(*(torch.as_tensor(a, dtype=torch.float64)[None, None] for a in PSMCParams.from_dm(per)))
    st = t[3].cpu().numpy()
    explicit = kern.interval_tracts(pp, np.arange(SMP_ROWS), intervals=t[:3], masks=np.abs(np.arange(SMP_K)[None, :] - st[:, None]) <= 2)
    assert torch.equal(sup.per_model, explicit.logp)
    wider = phlash_amd.segment_support(dms[0], data, t, slack=3, window_size=ws)
    assert bool((wider.logp >= sup.logp).all()) and bool((wider.logp > sup.logp).any())
    # two models: the logsumexp of the single-model calls; a time range is per model
    both = phlash_amd.segment_support(dms, data, t, slack=2, window_size=ws)
    each = torch.stack([phlash_amd.segment_support(d, data, t, slack=2, window_size=ws).logp for d in dms])
    assert both.per_model.shape == (2, len(t[0]))
    assert float((both.logp - (torch.logsumexp(each, 0) - np.log(2))).abs().max()) < 1e-12
    rng_ = phlash_amd.segment_support(dms, data, t, t_max=float(dm.eta.t[SMP_PREFIX]), window_size=ws)
    assert bool((rng_.logp <= 0).all()) and not bool(torch.isnan(rng_.logp).any())


@pytest.mark.gpu
def test_abi_refusals_and_the_device_side_check():
    import ctypes

    from phlash_amd import _lib

    rows, kern = _kernel16(False)
    eng = kern._eng
    lib = _lib.load()
    pa, inds, _, _ = kern._model_inputs(_bcast(_population(16, 3, seed=7)), np.arange(4))
    c = eng._sweep_call(pa, inds)
    dev = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int64, device=eng.device)  # noqa: E731
    off, st, en, mk = dev([0, 1, 1, 1, 1]), dev([0]), dev([5]), dev([3])
    ll = torch.zeros(3, 4, dtype=torch.float64, device=eng.device)
    lp = torch.zeros(3, 1, dtype=torch.float64, device=eng.device)
    torch.cuda.synchronize()

    def call(max_len=5, off=off.data_ptr(), st=st.data_ptr(), en=en.data_ptr(), mk=mk.data_ptr(), stride=0, lp=lp.data_ptr()):
        rc = lib.phk_interval_tracts(*c.head, *c.grid, kern.overlap, max_len, None, off, st, en, mk, stride, ll.data_ptr(), lp, c.stream)
        return rc, lib.phk_last_error().decode()

    for kw, words in ((dict(max_len=0), "max_len"), (dict(off=None), "iv_off"), (dict(st=None), "iv_start"), (dict(en=None), "iv_end"),
                      (dict(mk=None), "masks"), (dict(stride=-1), "mstride_b")):
        rc, msg = call(**kw)
        assert rc == _lib.PHK_EINVAL and words in msg, (kw, msg)
    torch.cuda.synchronize()
    assert not bool(ll.any()) and not bool(lp.any())  # nothing was enqueued
    rc, msg = call()
    assert rc == _lib.PHK_OK, msg
    assert not eng.underflow_risk() and bool(torch.isfinite(lp).all()) and bool((lp < 0).all())
    # an empty call computes ll only
    ll_e, lp_e = eng.interval_tracts(pa, inds, dev([0, 0, 0, 0, 0]), dev([]), dev([]), dev([]), warmup=kern.overlap, max_len=1)
    assert lp_e.shape == (3, 0) and torch.equal(ll_e, ll) and not eng.underflow_risk()
    # a list with an overlap, past the host's validation: the flag, and NaN for that row only
    iv = _lists16()
    order = np.lexsort((iv[1], iv[0]))
    r, s, e = (x[order] for x in iv)
    offs = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=4))])
    masks = dev(np.full(len(r), 0x0ff0))
    _, good = eng.interval_tracts(pa, inds, dev(offs), dev(s), dev(e), masks, warmup=kern.overlap, max_len=600, lens=dev(LENS16))
    assert not eng.underflow_risk()
    s_bad = s.copy()
    s_bad[offs[1] + 2] = e[offs[1] + 1] - 1  # row 1's third interval starts inside its second
    for plan in ((0, 4, 8, 4, 0), (1, 4, 16, 4, 4)):
        eng.set_plan(*plan)
        _, ref = eng.interval_tracts(pa, inds, dev(offs), dev(s), dev(e), masks, warmup=kern.overlap, max_len=600, lens=dev(LENS16))
        _, bad = eng.interval_tracts(pa, inds, dev(offs), dev(s_bad), dev(e), masks, warmup=kern.overlap, max_len=600, lens=dev(LENS16))
        with pytest.raises(AssertionError, match="interval list"):
            eng.underflow_risk()
        row1 = torch.as_tensor(r == 1, device=bad.device)
        assert bool(torch.isnan(bad[:, row1]).all()) and torch.equal(bad[:, ~row1], ref[:, ~row1]), plan
        # an interval longer than max_len is a bad list too
        _, short = eng.interval_tracts(pa, inds, dev(offs), dev(s), dev(e), masks, warmup=kern.overlap, max_len=599, lens=dev(LENS16))
        with pytest.raises(AssertionError, match="interval list"):
            eng.underflow_risk()
        long_rows = torch.as_tensor(r <= 1, device=bad.device)  # (rows 0 and 1 hold an interval of 600 windows each)
        assert bool(torch.isnan(short[:, long_rows]).all()) and torch.equal(short[:, ~long_rows], ref[:, ~long_rows]), plan
    del ctypes
