"""Posterior predictive simulation (phk_simulate / phlash_amd.simulate / simulate_rows / replicate_check).

CPU: the loop-form oracle (tests/simulate_oracle.py) against the exact law of (path, codes) by enumeration, the structured
draw rule against the dense matrix, the two statistics against a direct numpy computation, the host's statistics of the
data, the ABI's argument checks (no launch), the re-exports.
GPU: obs, paths, het and runs equal to the oracle's at every entry over K, L, bin, both parameter layouts and three masks;
the identities that tie calls to each other; a block without mass; the public layer.
Nothing here skips on a missing symbol: without phk_simulate every test fails.
"""

from __future__ import annotations

import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import sampling_oracle as so
import simulate_oracle as sim
from oracle import psmc_numpy as pn

GRID_B, GRID_S, GRID_R = 2, 3, 4
GRID_K = (2, 4, 5, 12, 16, 32, 64)
GRID_L = (1, 15, 16, 17, 65, 700)
GRID_BIN = (1, 7, 100)
GRID_SEED = 20241
LMAX = max(GRID_L)
MASKS = ("none", "holes", "lastbin")
OUTS = ("obs", "paths", "het", "runs")


def block(K, idx=0, theta=0.05):
    """default grid, theta = rho = 0.05 per window for idx = 0; the other blocks of a call differ a little"""
    return pn.from_dm(pn.default_dm(f"{K}*1", theta * (1.0 + 0.1 * idx), theta * (1.0 + 0.07 * idx)))


def grid_blocks(K, layout):
    """[B][S or 1] blocks: one per particle ("bcast", pstride_s = 0) or one per (particle, row) ("rows")"""
    if layout == "bcast":
        return [[block(K, b)] for b in range(GRID_B)]
    return [[block(K, b * GRID_S + s) for s in range(GRID_S)] for b in range(GRID_B)]


@functools.lru_cache(maxsize=None)
def grid_reference(K, layout, B=GRID_B, n_rep=GRID_R, seed=GRID_SEED, seq0=0):
    """(paths uint8 [B, S, n_rep, LMAX], codes int8 likewise, margins of the two) of the grid's call at L = LMAX, computed once
    and shared, read only: the generator is counter-based, so a call at L < LMAX is the first L sites of this one"""
    blocks = grid_blocks(K, layout)
    shape = (B, GRID_S, n_rep, LMAX)
    paths, codes, mp, mo = np.empty(shape, np.uint8), np.empty(shape, np.int8), np.empty(shape), np.empty(shape)
    for b in range(B):
        for s in range(GRID_S):
            out = sim.simulate_paths(blocks[b][s if layout == "rows" else 0], LMAX, np.full(n_rep, seq0 + b * GRID_S + s), np.arange(n_rep), seed)
            assert not out["flag"]
            paths[b, s], codes[b, s], mp[b, s], mo[b, s] = out["paths"], out["codes"], out["m_path"], out["m_obs"]
    for a in (paths, codes, mp, mo):
        a.setflags(write=False)
    return paths, codes, mp, mo


def grid_mask(kind, L):
    """int8 [S, L] (0 / -1) or None"""
    if kind == "none":
        return None
    m = np.zeros((GRID_S, L), np.int8)
    if kind == "holes":  # isolated missing sites in every row and a run of 120 (clipped to the row)
        g = np.random.default_rng(L)
        for s in range(GRID_S):
            m[s, g.integers(0, L, size=max(1, L // 12))] = -1
        m[1, L // 3 : L // 3 + 120] = -1
    else:  # row 1's mask covers its last bin, whichever of the grid's bins is asked for
        m[1, 100 * ((L - 1) // 100) :] = -1
    return m


def params_tensor(blocks):
    return torch.as_tensor(np.stack([np.stack([q.stack() for q in row]) for row in blocks])).cuda()  # [B, S or 1, 7, K]


def raw_call(P, S, n_rep, L, seed=GRID_SEED, seq0=0, mask=None, want=OUTS, bin=1, stride=None, sentinel=None):
    """phk_simulate through ctypes on buffers of the test's own -> dict of numpy arrays (full row stride) and ``flags``"""
    from phlash_amd import _lib

    lib = _lib.load()
    B, Sp, _, K = P.shape
    stride = -(-L // 16) * 16 if stride is None else stride
    nbin = -(-L // bin)
    fill = 0 if sentinel is None else sentinel
    bufs = {"obs": torch.full((B, S, n_rep, stride), fill, dtype=torch.int8, device="cuda"),
            "paths": torch.full((B, S, n_rep, stride), fill, dtype=torch.uint8, device="cuda"),
            "het": torch.full((B, S, n_rep, nbin), -7, dtype=torch.int32, device="cuda"),
            "runs": torch.full((B, S, n_rep, 32), -7, dtype=torch.int32, device="cuda")}
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    m = None if mask is None else torch.as_tensor(mask).cuda().contiguous()
    ptr = lambda k: bufs[k].data_ptr() if k in want else None  # noqa: E731
    rc = lib.phk_simulate(0, K, P.data_ptr(), P.stride(0), 0 if Sp == 1 else P.stride(1), B, S, n_rep, L, ctypes.c_uint64(seed), seq0,
                          None if m is None else m.data_ptr(), 0 if m is None else m.stride(0), ptr("obs"), ptr("paths"), stride, bin,
                          ptr("het"), ptr("runs"), flags.data_ptr(), None)
    assert rc == _lib.PHK_OK, lib.phk_last_error()
    torch.cuda.synchronize()
    out = {k: bufs[k].cpu().numpy() for k in want}
    out["flags"] = int(flags.item())
    return out


def expected(paths, codes, mask, L, bin):
    """the oracle's four outputs [B, S, n_rep, ...] of a call at L sites under ``mask``"""
    B, S, R = paths.shape[:3]
    obs = np.stack([np.stack([sim.lay_mask(codes[b, s, :, :L], None if mask is None else mask[s]) for s in range(S)]) for b in range(B)])
    het, runs = sim.statistics(obs.reshape(-1, L), bin)
    return obs, paths[..., :L], het.reshape(B, S, R, -1), runs.reshape(B, S, R, 32)


def assert_same(got, want, margins, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        i = tuple(bad[0])
        m = f", the oracle's margin there {margins[i]:.3e}" if margins is not None and margins.shape == got.shape else ""
        raise AssertionError(f"{what}: {len(bad)} entries differ, first at {i}: got {got[i]}, oracle {want[i]}{m}")


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("K,L,masked", [(3, 4, ()), (3, 4, (2,)), (2, 3, ()), (2, 3, (0,))])
def test_oracle_matches_the_exact_law_by_enumeration(K, L, masked):
    N = 20_000
    pp = block(K)
    out = sim.simulate_paths(pp, L, np.full(N, 5), np.arange(N), seed=11, margins=False)
    mask = np.zeros(L, np.int8)
    mask[list(masked)] = -1
    obs = sim.lay_mask(out["codes"], mask)
    law = sim.exact_law(pp, L, masked)
    assert abs(sum(law.values()) - 1.0) < 1e-12
    seen = {}
    for a in range(N):
        key = (tuple(int(x) for x in out["paths"][a]), tuple(int(x) for x in obs[a]))
        seen[key] = seen.get(key, 0) + 1
    assert set(seen) <= set(law), "a drawn (path, codes) pair has probability zero"
    keys = sorted(law)
    score = so.frequency_score([seen.get(k, 0) / N for k in keys], [law[k] for k in keys], N)
    print(f"K={K} L={L} masked={masked}: {len(seen)} of {len(keys)} outcomes seen, score {score:.3f}")
    assert score < 1.0


@pytest.mark.parametrize("K,min_rows", [(4, 2), (16, 10), (64, 40)])
def test_structured_rule_against_the_dense_matrix(K, min_rows):
    """theta = rho = 0.05 on the default grid, seed 77, q = 3, 64 replicates x 4,000 sites: the transition frequencies out of
    every state with more than 200 visits against the normalised rows of dense_from_pp, the het frequency by state against
    emis1 / (emis0 + emis1), and the chain drawn from the dense matrix's own row-wise cumsum with the same uniforms."""
    R, L = 64, 4000
    pp = block(K)
    out = sim.simulate_paths(pp, L, np.full(R, 3), np.arange(R), seed=77, margins=False)
    paths, codes = out["paths"].astype(int), out["codes"]
    A = pn.dense_from_pp(pp)
    A = A / A.sum(1, keepdims=True)
    counts = np.zeros((K, K))
    np.add.at(counts, (paths[:, :-1].ravel(), paths[:, 1:].ravel()), 1)
    visits = counts.sum(1)
    rows = np.flatnonzero(visits > 200)
    score = max(so.frequency_score(counts[i] / visits[i], A[i], visits[i]) for i in rows)
    ph = np.asarray(pp.emis1) / (np.asarray(pp.emis0) + np.asarray(pp.emis1))
    n_state = np.bincount(paths.ravel(), minlength=K)
    states = np.flatnonzero(n_state > 200)
    het_score = max(so.frequency_score([codes[paths == k].mean()], [ph[k]], n_state[k]) for k in states)
    dpaths, dcodes = sim.dense_simulate(pp, L, np.full(R, 3), np.arange(R), seed=77)
    differ = float((dpaths != paths).mean())
    print(f"K={K}: transition score {score:.3f} over {len(rows)} rows, het score {het_score:.3f}, dense chain differs at {differ:.2e} of the sites")
    assert len(rows) >= min_rows, len(rows)
    assert score < 1.0 and het_score < 1.0
    assert differ < 1e-3  # the two rules part only where a draw falls within a rounding of a boundary


def _direct_statistics(obs, bin):
    """numpy, no site loop: hets by reduceat over the bins, runs from the edges of the hom indicator"""
    obs = np.asarray(obs)
    n, L = obs.shape
    het = np.add.reduceat((obs == 1).astype(np.int32), np.arange(0, L, bin), axis=1)
    runs = np.zeros((n, 32), np.int32)
    for a in range(n):
        hom = np.concatenate([[False], obs[a] == 0, [False]])
        starts, ends = np.flatnonzero(~hom[:-1] & hom[1:]), np.flatnonzero(hom[:-1] & ~hom[1:])
        for length in ends - starts:
            runs[a, int(length).bit_length() - 1] += 1
    return het, runs


def test_statistics_against_a_direct_computation():
    # hand-made rows: a run that touches the row's end, one cut by a missing site, length 1, lengths 8 and 16 exactly
    row = np.array([1] + [0] * 8 + [1] + [0] + [1] + [0] * 5 + [-1] + [0] * 16 + [1, 1] + [0] * 3, np.int8)
    het, runs = sim.statistics(row[None], 7)
    want = np.zeros(32, int)
    for length in (8, 1, 5, 16, 3):
        want[int(np.floor(np.log2(length)))] += 1
    assert runs[0].tolist() == want.tolist() and runs[0, 3] == 1 and runs[0, 4] == 1 and runs[0, 0] == 1
    assert het.sum() == 5 and het.shape == (1, -(-len(row) // 7))
    all_hom = np.zeros((1, 64), np.int8)  # one run, the whole row, a power of two
    assert sim.statistics(all_hom, 100)[1][0, 6] == 1 and sim.statistics(all_hom, 100)[0].tolist() == [[0]]
    # the oracle's own rows under a mask, every bin of the grid
    out = sim.simulate_paths(block(16), 700, np.full(6, 2), np.arange(6), seed=5, margins=False)
    obs = sim.lay_mask(out["codes"], grid_mask("holes", 700)[1])
    for bin in GRID_BIN + (700, 1000):
        h, r = sim.statistics(obs, bin)
        dh, dr = _direct_statistics(obs, bin)
        assert np.array_equal(h, dh) and np.array_equal(r, dr), bin
        assert r.sum() > 0 and r[:, 10:].sum() == 0  # no run of 1,024 sites in 700


def test_planted_misfit_shows_in_the_run_spectrum():
    """Through the oracle alone.  One row of 6,000 windows from ``synth.simulate_chunks`` (K = 16, theta = rho = 0.05 per window,
    1 % missing, data seed 1) under a bottleneck, c = 25 in states 3 .. 7 of the default grid; 60 replicates (seed 1, q = 0) under
    the row's own mask from the true model and from the constant-size model; buckets 0 .. 7 (runs of 1 .. 255 windows: the data
    has runs in every one of them, 4 / 6 / 11 / 12 / 13 / 21 / 20 / 9).  Observed ``runs`` p-values, chosen on the CPU:
        true model   0.25 0.18 0.22 0.22 0.47 0.18 0.27 0.87   -- none outside [0.01, 0.99]
        constant     1.00 1.00 1.00 1.00 1.00 0.98 0.00 0.00   -- seven outside: too few short runs, too many long ones
    (data seeds 2 .. 4 and replicate seed 2 show the same picture; from bucket 8 on the data has at most three runs or none and
    p = 1 means nothing there)."""
    from phlash_amd.synth import simulate_chunks

    K, L, R, theta = 16, 6000, 60, 0.05
    c = np.ones(K)
    c[3:8] = 25.0
    dm = pn.default_dm(f"{K}*1", theta, theta)
    models = {"true": pn.from_dm(pn.DM(dm.t, c, theta, theta)), "constant": pn.from_dm(dm)}
    data = simulate_chunks(K, 1, L, seed=1, theta=theta, rho=theta, missing=0.01, c=c)
    runs_data = sim.statistics(data, 100)[1][0]
    assert (runs_data[:8] > 0).all()
    p = {}
    for name, pp in models.items():
        out = sim.simulate_paths(pp, L, np.zeros(R, int), np.arange(R), seed=1, margins=False)
        runs = sim.statistics(sim.lay_mask(out["codes"], data[0]), 100)[1]
        p[name] = (runs >= runs_data[None]).mean(0)[:8]
        print(name, np.round(p[name], 2).tolist())
    assert ((p["true"] >= 0.01) & (p["true"] <= 0.99)).all()
    assert ((p["constant"] < 0.01) | (p["constant"] > 0.99)).sum() >= 1


def test_host_statistics_of_the_data():
    from phlash_amd.simulate import data_statistics

    g = np.random.default_rng(3)
    rows = (g.random((4, 333)) < 0.1).astype(np.int8)
    rows.flat[g.integers(0, rows.size, 40)] = -1
    rows[2, 100:250] = 0
    rows[3] = -1
    for bin in (1, 7, 100, 500):
        h, r = data_statistics(rows, bin)
        dh, dr = sim.statistics(rows, bin)
        assert np.array_equal(h, dh) and np.array_equal(r, dr), bin


def test_argument_errors_without_a_launch():
    from phlash_amd import _lib

    lib = _lib.load()
    ok = dict(device=0, K=16, params=1024, pb=112, ps=0, B=2, S=3, n_rep=4, L=100, seed=1, seq0=0, mask=2048, mask_stride=112, obs=4096,
              paths=8192, row_stride=112, bin=7, het=256, runs=512, flags=64)  # (fake addresses: nothing is read before the checks)
    bad = [dict(K=1), dict(K=65), dict(B=0), dict(S=0), dict(n_rep=0), dict(L=0), dict(n_rep=65536), dict(L=2 ** 32 - 1, row_stride=2 ** 32, mask_stride=2 ** 32),
           dict(params=None), dict(flags=None), dict(obs=None, paths=None, het=None, runs=None), dict(bin=0), dict(row_stride=96), dict(mask_stride=99),
           dict(row_stride=120), dict(obs=4100), dict(paths=8200)]
    for change in bad:
        a = {**ok, **change}
        rc = lib.phk_simulate(a["device"], a["K"], a["params"], a["pb"], a["ps"], a["B"], a["S"], a["n_rep"], a["L"], ctypes.c_uint64(a["seed"]),
                              a["seq0"], a["mask"], a["mask_stride"], a["obs"], a["paths"], a["row_stride"], a["bin"], a["het"], a["runs"], a["flags"], None)
        assert rc == _lib.PHK_EINVAL, (change, rc, lib.phk_last_error())
    # what the rules leave alone: bin is not read without het, row_stride not without obs / paths -- checked on the GPU, where the call runs


def test_lazy_exports():
    import phlash_amd
    from phlash_amd import simulate as mod

    assert phlash_amd.simulate_rows is mod.simulate_rows and phlash_amd.replicate_check is mod.replicate_check
    assert phlash_amd.Simulated is mod.Simulated and phlash_amd.ReplicateCheck is mod.ReplicateCheck


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("L", GRID_L)
@pytest.mark.parametrize("K", GRID_K)
def test_equal_to_the_oracle_at_every_entry(K, L):
    for layout in ("bcast", "rows"):
        paths, codes, mp, mo = grid_reference(K, layout)
        P = params_tensor(grid_blocks(K, layout))
        for kind in MASKS:
            mask = grid_mask(kind, L)
            for bin in GRID_BIN:
                got = raw_call(P, GRID_S, GRID_R, L, mask=mask, bin=bin)
                obs, pth, het, runs = expected(paths, codes, mask, L, bin)
                what = f"K={K} L={L} {layout} mask={kind} bin={bin}"
                assert_same(got["paths"][..., :L], pth, mp[..., :L], what + " paths")
                assert_same(got["obs"][..., :L], obs, mo[..., :L], what + " obs")
                assert_same(got["het"], het, None, what + " het")
                assert_same(got["runs"], runs, None, what + " runs")
                assert got["flags"] == 0, what


@pytest.mark.gpu
def test_identities():
    K, L, bin = 16, 700, 7
    P = params_tensor(grid_blocks(K, "rows"))
    mask = grid_mask("holes", L)
    full = raw_call(P, GRID_S, GRID_R, L, mask=mask, bin=bin, stride=736, sentinel=0x55)
    assert full["flags"] == 0
    # positions >= L of every row keep what was there
    assert (full["obs"][..., L:] == 0x55).all() and (full["paths"][..., L:] == 0x55).all()
    # any subset of the outputs: the same bytes
    for n in range(1, 4):
        for want in itertools.combinations(OUTS, n):
            part = raw_call(P, GRID_S, GRID_R, L, mask=mask, bin=bin, want=want, stride=736, sentinel=0x55)
            assert part["flags"] == 0
            for k in want:
                assert np.array_equal(part[k], full[k]), (want, k)
    # replicate r does not depend on n_rep
    nine = raw_call(P, GRID_S, 9, L, mask=mask, bin=bin)
    for k in OUTS:
        a = nine[k][:, :, :GRID_R]
        assert np.array_equal(a[..., :L] if k in ("obs", "paths") else a, full[k][..., :L] if k in ("obs", "paths") else full[k]), k
    # slabs over particles with seq0
    for b in range(GRID_B):
        one = raw_call(P[b : b + 1], GRID_S, GRID_R, L, mask=mask, bin=bin, seq0=b * GRID_S, stride=736, sentinel=0x55)
        assert one["flags"] == 0
        for k in OUTS:
            assert np.array_equal(one[k][0], full[k][b]), (b, k)
    # the seed
    again = raw_call(P, GRID_S, GRID_R, L, mask=mask, bin=bin, stride=736, sentinel=0x55)
    other = raw_call(P, GRID_S, GRID_R, L, mask=mask, bin=bin, seed=GRID_SEED + 1, stride=736, sentinel=0x55)
    for k in OUTS:
        assert np.array_equal(again[k], full[k]), k
        assert not np.array_equal(other[k], full[k]), k
    # the mask is laid over the output only
    bare = raw_call(P, GRID_S, GRID_R, L, bin=bin, stride=736, sentinel=0x55)
    assert bare["flags"] == 0
    assert np.array_equal(bare["paths"], full["paths"])
    miss = np.broadcast_to((mask < 0)[None, :, None, :], full["obs"][..., :L].shape)
    assert (full["obs"][..., :L][miss] == -1).all() and np.array_equal(full["obs"][..., :L][~miss], bare["obs"][..., :L][~miss])
    assert (bare["obs"][..., :L] >= 0).all()
    het, runs = sim.statistics(full["obs"][..., :L].reshape(-1, L), bin)
    assert np.array_equal(het.reshape(full["het"].shape), full["het"]) and np.array_equal(runs.reshape(full["runs"].shape), full["runs"])
    # without het, bin is not read; without obs / paths, neither is row_stride
    lone = raw_call(P, GRID_S, GRID_R, L, mask=mask, bin=1, want=("runs",), stride=16)
    assert np.array_equal(lone["runs"], full["runs"]) and lone["flags"] == 0


@pytest.mark.gpu
def test_a_block_without_mass_sets_the_flag():
    K, L = 4, 40
    good = block(K)
    rows = good.stack()
    rows[:4, 0] = 0.0  # b, d, u, v of state 0
    rows[6] = [1.0, 0.0, 0.0, 0.0]  # pi: every chain starts in state 0, whose row has no mass
    dead = pn.PP(*rows)
    ref = sim.simulate_paths(dead, L, np.full(3, 1), np.arange(3), seed=GRID_SEED)
    assert ref["flag"] and (ref["paths"] == 0).all()
    P = torch.as_tensor(np.stack([good.stack(), rows]))[:, None].cuda()  # particle 0 is sound
    got = raw_call(P, 1, 3, L, bin=5)  # (raw_call asserts PHK_OK)
    assert got["flags"] & 1
    assert np.array_equal(got["paths"][1, 0, :, :L], ref["paths"]) and np.array_equal(got["obs"][1, 0, :, :L], ref["codes"])
    sound = sim.simulate_paths(good, L, np.full(3, 0), np.arange(3), seed=GRID_SEED)
    assert np.array_equal(got["paths"][0, 0, :, :L], sound["paths"]) and np.array_equal(got["obs"][0, 0, :, :L], sound["codes"])
    assert raw_call(P[:1], 1, 3, L, bin=5)["flags"] == 0


def _public_inputs():
    from phlash_amd.size_history import DemographicModel

    g = np.random.default_rng(8)
    contigs = [(g.random((2, 300)) < 0.05).astype(np.int8), (g.random((1, 170)) < 0.05).astype(np.int8)]
    for c in contigs:
        c.flat[g.integers(0, c.size, 15)] = -1
    contigs[0][1, 40:160] = -1
    dms = [DemographicModel.default("16*1", 5e-4, 5e-4), DemographicModel.default("16*1", 7e-4, 4e-4)]
    return dms, contigs


def _public_blocks(dms, window_size=100):
    from phlash_amd.params import PSMCParams
    from phlash_amd.size_history import DemographicModel

    per = [DemographicModel(eta=m.eta, theta=float(m.theta) * window_size, rho=float(m.rho) * window_size) for m in dms]
    return [pn.PP(*(np.asarray(getattr(PSMCParams.from_dm(m), f), float) for f in pn.PP._fields)) for m in per]


@pytest.mark.gpu
def test_simulate_rows_on_ragged_contigs():
    import phlash_amd

    dms, contigs = _public_inputs()
    R, seed = 3, 99
    out = phlash_amd.simulate_rows(dms, contigs, n_rep=R, seed=seed, paths=True)
    assert isinstance(out, phlash_amd.Simulated) and len(out.obs) == 2 and len(out.paths) == 2
    blocks = _public_blocks(dms)
    N, row0 = 3, 0
    for c, obs, paths in zip(contigs, out.obs, out.paths):
        n, length = c.shape
        assert obs.shape == (2, n, R, length) and obs.dtype == torch.int8 and paths.dtype == torch.uint8 and obs.is_cuda
        for b in range(2):
            for s in range(n):
                ref = sim.simulate(blocks[b], length, b * N + row0 + s, R, seed, mask_row=c[s])
                assert np.array_equal(obs[b, s].cpu().numpy(), ref["obs"]) and np.array_equal(paths[b, s].cpu().numpy(), ref["paths"]), (b, s)
        row0 += n
    # no data: one unmasked row of n_sites windows; a single model is a list of one
    free = phlash_amd.simulate_rows(dms[0], n_sites=90, n_rep=2, seed=seed)
    assert free.paths is None and free.obs.shape == (1, 1, 2, 90)
    assert np.array_equal(free.obs[0, 0].cpu().numpy(), sim.simulate(blocks[0], 90, 0, 2, seed)["obs"])


@pytest.mark.gpu
def test_replicate_check_against_the_stored_rows():
    import phlash_amd

    dms, contigs = _public_inputs()
    data = np.full((3, 300), -1, np.int8)
    data[:2] = contigs[0]
    data[2, :170] = contigs[1][0]
    R, bin, seed = 8, 50, 5
    chk = phlash_amd.replicate_check(dms, data, n_rep=R, bin=bin, seed=seed)
    rows = phlash_amd.simulate_rows(dms, data, n_rep=R, seed=seed).obs.cpu().numpy()  # [B, N, R, L]
    B, N, _, L = rows.shape
    het, runs = sim.statistics(rows.reshape(-1, L), bin)
    het_data, runs_data = sim.statistics(data, bin)
    for name, x, dat in (("het", het.reshape(B, N, R, -1), het_data), ("runs", runs.reshape(B, N, R, 32), runs_data)):
        x = np.moveaxis(x, 1, 0).reshape(N, B * R, -1)
        lo, hi = np.quantile(x, [0.025, 0.975], axis=1)
        assert np.array_equal(getattr(chk, name + "_data"), dat), name
        assert np.array_equal(getattr(chk, name + "_mean"), x.mean(1)) and np.array_equal(getattr(chk, name + "_lo"), lo), name
        assert np.array_equal(getattr(chk, name + "_hi"), hi) and np.array_equal(getattr(chk, name + "_p"), (x >= dat[:, None]).mean(1)), name
    assert chk.het_mean.shape == (3, 6) and chk.runs_p.shape == (3, 32)
    # a byte cap of one model's buffers: two slabs, the same numbers
    two = phlash_amd.replicate_check(dms, data, n_rep=R, bin=bin, seed=seed, max_stat_bytes=N * R * (6 + 32) * 4)
    for a, b in zip(chk, two):
        assert np.array_equal(a, b)
    # a list of contigs: per-contig arrays cut to the contig's bins
    per = phlash_amd.replicate_check(dms, contigs, n_rep=R, bin=bin, seed=seed)
    assert per.het_mean[0].shape == (2, 6) and per.het_mean[1].shape == (1, 4) and per.runs_p[1].shape == (1, 32)
    assert np.array_equal(per.het_mean[0], chk.het_mean[:2]) and np.array_equal(per.het_p[1], chk.het_p[2:, :4])
