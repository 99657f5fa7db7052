"""Posterior predictive simulation (phk_simulate) on seeded random draws (tests/simulate_fuzz.py): every buffer a call leaves
behind equal to the float64 loop-form oracle's at every entry.

CPU: the coverage of the default seeds (sequences per parameter block around the workgroup size, the vector and the scalar
mask load past the first block, 64-bit counters, blocks without mass, every kernel instantiation), and the comparator against
the oracle's own output with one fault injected.  GPU: one call per draw through ctypes on buffers of the test's own (mask
views and row strides included), a repeat call for the same bytes, and ``simulate_rows`` with 70 replicates.
``pytest -s -m gpu tests/test_simulate_fuzz.py`` prints one ``fuzz`` line per draw and a summary (profiles/simulate_fuzz.txt).
"""

from __future__ import annotations

import ctypes
import os
import time

import numpy as np
import pytest

import simulate_fuzz as zf
import simulate_oracle as sim

DEFAULT_SEEDS = 49  # the smallest count that draws the whole list of test_default_seeds_cover_the_list; that test checks it
# draws that found a bug, kept by name whatever the number of seeds run: name -> seed
REGRESSIONS: dict = {}
N_SEEDS = int(os.environ.get("PHK_SIMULATE_FUZZ_SEEDS", str(DEFAULT_SEEDS)))


def _defaults():
    return [zf.draw(seed) for seed in range(DEFAULT_SEEDS)]


# ------------------------------------------------------------------------------------------------- CPU
def _features(d):
    f = {f"K={d.K}", f"n_rep={d.n_rep}", f"L={d.L}" if d.L in (1, 2, 15, 16, 17, 31, 32, 33) else "L>=48", f"scale={d.scale}",
         f"seq0={d.seq0}", f"mask {d.mask_kind}", "seed high word " + ("set" if d.key >> 32 else "0")}
    n = d.per_block
    if d.per_row:
        f.add("rows: " + ("below 64" if n < 64 else "exactly 64" if n == 64 else "65..128, last workgroup partly filled" if n < 128 else "above 128"))
    else:
        f.add("bcast")
        if any(e % d.n_rep for e in range(zf.NT, n, zf.NT)):
            f.add("bcast: a workgroup boundary inside one row's replicates")
    if n > zf.NT and n % zf.NT:
        f.add("a partly filled last workgroup")
    rows, stats = bool({"obs", "paths"} & set(d.want)), bool({"het", "runs"} & set(d.want))
    kern = "rows + stats" if rows and stats else "rows" if rows else "stats"
    f.add(f"kernel {kern}")
    f |= {f"want {k}" for k in d.want}
    if n > zf.NT:  # every instantiation past one workgroup per block, and with the vector mask load past the first block
        f.add(f"kernel {kern}, more than one workgroup per block")
    if d.mask is not None and d.store == "aligned" and d.L >= 33:
        f.add(f"kernel {kern}, aligned mask, L >= 33")
    if d.seq0 >= 2 ** 32 and d.key >> 32:
        f.add("seq0 >= 2^32 with the seed's high word set")
    if d.mask is not None and d.L >= 32:
        f.add("aligned mask, two full blocks" if d.store == "aligned" else "misaligned mask, two full blocks")
        if d.store == "aligned" and d.L >= 33:
            f.add("aligned mask, L >= 33")
        f.add(f"mask store {d.store}")
    if d.stride > zf.ceil16(d.L):
        f.add("row stride above ceil16(L)")
    f.add(f"bin {'1' if d.bin == 1 else 'L' if d.bin == d.L else 'L+5' if d.bin == d.L + 5 else 'inside'}")
    o = zf.oracle(d)
    if d.special == "dead_state" and o["flag"]:
        p = o["paths"][-1].reshape(-1, d.L)
        if ((p[:, 0] != d.dead) & (p == d.dead).any(1)).any():
            f.add("a state without mass reached mid-chain")
    if d.special == "dead_emission" and o["flag"]:
        f.add("an emission row without mass, visited")
    if d.special == "pi_last":
        f.add("pi on the last state")
    if d.special == "none" and not o["flag"]:
        f.add("sound blocks, no flag")
    return f


def _wanted():
    want = {f"K={K}" for K in zf.KS} | {f"n_rep={n}" for n in zf.NREPS} | {f"L={L}" for L in (1, 2, 15, 16, 17, 31, 32, 33)} | {"L>=48"}
    want |= {f"scale={s}" for s in zf.SCALES} | {f"seq0={q}" for q in zf.SEQ0S} | {f"mask {m}" for m in zf.MASKS}
    want |= {"seed high word set", "seed high word 0", "rows: below 64", "rows: exactly 64", "rows: 65..128, last workgroup partly filled",
             "rows: above 128", "bcast", "bcast: a workgroup boundary inside one row's replicates", "a partly filled last workgroup",
             "kernel rows + stats", "kernel rows", "kernel stats", "aligned mask, two full blocks", "misaligned mask, two full blocks",
             "aligned mask, L >= 33", "mask store offset", "mask store tight", "row stride above ceil16(L)", "bin 1", "bin L", "bin L+5",
             "bin inside", "a state without mass reached mid-chain", "an emission row without mass, visited", "pi on the last state",
             "sound blocks, no flag"}
    want |= {f"want {k}" for k in zf.OUTS} | {"seq0 >= 2^32 with the seed's high word set"}
    want |= {f"kernel {k}, {w}" for k in ("rows + stats", "rows", "stats") for w in ("more than one workgroup per block", "aligned mask, L >= 33")}
    return want


def first_covering_count(limit=128):
    want, seen = _wanted(), set()
    for seed in range(limit):
        seen |= _features(zf.draw(seed))
        if not want - seen:
            return seed + 1
    return None


def test_default_seeds_cover_the_list():
    seen = set()
    for d in _defaults():
        seen |= _features(d)
        assert d.B * d.S * d.n_rep * d.L <= zf.MAX_STEPS
    want = _wanted()
    assert not want - seen, f"the default seeds never draw: {sorted(want - seen)}"
    assert DEFAULT_SEEDS <= 128
    assert first_covering_count(DEFAULT_SEEDS) == DEFAULT_SEEDS, "DEFAULT_SEEDS is not the smallest count that covers the list"


def _first(pred):
    for d in _defaults():
        if pred(d):
            return d
    raise AssertionError("no default draw fits: change the draw")


def _pow2_low_statistics(obs, bin):
    """the statistics with a run of exactly 2^k sites (k >= 1) counted in bucket k - 1"""
    het, runs = sim.statistics(obs, bin)
    runs = np.zeros_like(runs)
    for a in range(obs.shape[0]):
        run = 0
        for c in list(obs[a]) + [1]:
            if c == 0:
                run += 1
            elif run:
                runs[a, max((run - 1).bit_length() - 1, 0) if run & (run - 1) == 0 else run.bit_length() - 1] += 1
                run = 0
    return het, runs


def test_comparator_catches_seeded_faults():
    """The oracle's own output passes on every default draw; with one fault injected it fails."""
    caught = []

    def check(d, name, obs=None, paths=None, het=None, runs=None, flag=None, edit=None):
        o = zf.oracle(d)
        assert zf.compare(d, zf.oracle_candidate(d)) is None
        if obs is not None and het is None:
            het, runs = zf.stats(obs, d.bin)  # (the statistics follow the rows the kernel reports)
        pick = lambda x, k: o[k] if x is None else x  # noqa: E731
        cand = zf.buffers(d, pick(obs, "obs"), pick(paths, "paths"), pick(het, "het"), pick(runs, "runs"), o["flag"] if flag is None else flag)
        if edit is not None:
            edit(cand)
        msg = zf.compare(d, cand)
        print(f"simulate fault '{name}' on seed {d.seed}: {msg}")
        assert msg is not None, name
        caught.append(name)

    def wrapped(d):
        """every output of the sequence at index idx >= 64 of its parameter block taken from index idx - 64"""
        o = zf.oracle(d)
        out = {}
        for k in ("obs", "paths"):
            x = o[k].copy()
            flat = x.reshape(d.B, d.S * d.n_rep, d.L) if not d.per_row else x.reshape(d.B * d.S, d.n_rep, d.L)
            flat[:, zf.NT :] = flat[:, : -zf.NT].copy()
            out[k] = x
        return out

    for name, pred in (("rows", lambda d: d.per_row and d.n_rep > zf.NT), ("bcast", lambda d: not d.per_row and d.per_block > zf.NT)):
        d = _first(lambda d: pred(d) and not zf.oracle(d)["flag"] and d.L >= 15)
        check(d, f"a replicate index wrapped at the workgroup size ({name})", **wrapped(d))
    masked = lambda d: d.mask is not None and d.mask_kind == "holes" and set(d.want) & {"obs", "het", "runs"}  # noqa: E731
    d = _first(lambda d: masked(d) and d.L >= 15)
    check(d, "the mask shifted one site", obs=zf.lay(zf.oracle(d)["codes"], np.roll(d.mask, 1, axis=1)))
    d = _first(lambda d: masked(d) and d.L >= 33)
    m = d.mask.copy()
    m[:, 16 : d.L // 16 * 16] = d.mask[:, : d.L // 16 * 16 - 16]
    assert not np.array_equal(m, d.mask)
    check(d, "a mask block read at the wrong t0", obs=zf.lay(zf.oracle(d)["codes"], m))
    d = _first(lambda d: {"obs", "paths"} <= set(d.want) and d.L >= 15)
    o = zf.oracle(d)
    check(d, "obs and paths swapped", obs=o["paths"].astype(np.int8), paths=o["obs"].astype(np.uint8), het=o["het"], runs=o["runs"])
    pow2 = lambda d: "runs" in d.want and (zf.oracle(d)["runs"] != zf.stats(zf.oracle(d)["obs"], d.bin, _pow2_low_statistics)[1]).any()  # noqa: E731
    d = _first(pow2)
    check(d, "a run of exactly 2^k sites counted in bucket k - 1", runs=zf.stats(zf.oracle(d)["obs"], d.bin, _pow2_low_statistics)[1])
    shift = lambda x: np.concatenate([x[..., 1:], np.zeros_like(x[..., :1])], -1)  # noqa: E731
    d = _first(lambda d: "het" in d.want and 1 < d.bin < d.L and (zf.stats(shift(zf.oracle(d)["obs"]), d.bin)[0] != zf.oracle(d)["het"]).any())
    o = zf.oracle(d)
    shifted = shift(o["obs"])
    check(d, "het bins shifted by one site", het=zf.stats(shifted, d.bin)[0], runs=o["runs"])
    d = _first(lambda d: zf.oracle(d)["flag"])
    check(d, "the flag missing", flag=False)
    d = _first(lambda d: not zf.oracle(d)["flag"])
    check(d, "a flag without a cause", flag=True)
    d = _first(lambda d: "obs" in d.want)
    check(d, "a byte written past L", edit=lambda c: c["obs"].__setitem__((-1, -1, -1, d.L), 0))
    d = _first(lambda d: "paths" not in d.want)
    check(d, "a buffer that was not asked for written", edit=lambda c: c["paths"].__setitem__((0, 0, 0, 0), 0))
    assert len(caught) == 11
    for d in _defaults():
        assert zf.compare(d, zf.oracle_candidate(d)) is None, zf.describe(d)


# ------------------------------------------------------------------------------------------------- GPU
STATS: list = []


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if not STATS:
        return
    print("\nsimulate fuzz summary")
    print(f"  simulate: {len(STATS)} draws equal to the oracle at every entry ({sum(r['entries'] for r in STATS)} entries compared), "
          f"{sum(r['flag'] for r in STATS)} of them with the flag raised")
    print(f"  wall time of test_simulate_random_shapes: {sum(r['time'] for r in STATS):.1f} s (oracles included)")


def _mask_tensor(d):
    """the draw's mask on the device as the draw stores it -> (tensor [S, >= L] or None); -1 wherever the call must not read"""
    import torch

    if d.mask is None:
        return None
    m = torch.as_tensor(d.mask)
    if d.store == "aligned":
        buf = torch.full((d.S, zf.ceil16(d.L) + 16), -1, dtype=torch.int8, device="cuda")
        view = buf[:, : zf.ceil16(d.L)] if d.seed % 2 else buf  # (a row stride of ceil16(L) + 16 either way)
        assert view.data_ptr() % 16 == 0 and view.stride(0) % 16 == 0
    elif d.store == "offset":
        stride = d.L + int(d.seed % 3) * 8
        buf = torch.full((1 + d.S * stride,), -1, dtype=torch.int8, device="cuda")
        view = buf[1:].view(d.S, stride)
        assert view.data_ptr() % 16 == 1
    else:
        view = torch.full((d.S, d.L), -1, dtype=torch.int8, device="cuda")
        assert view.stride(0) % 16 != 0
    view[:, : d.L] = m.cuda()
    return view


def raw_call(d, P, mask):
    """phk_simulate through ctypes on buffers of the test's own (tests/test_simulate.raw_call, with the mask as a view of any
    pointer and stride, the row stride and the fills of the draw) -> the buffers as simulate_fuzz.buffers lays them out"""
    import torch

    from phlash_amd import _lib

    lib = _lib.load()
    B, Sp, _, K = P.shape
    shape = (d.B, d.S, d.n_rep)
    bufs = {"obs": torch.full(shape + (d.stride,), zf.SENTINEL, dtype=torch.int8, device="cuda"),
            "paths": torch.full(shape + (d.stride,), zf.SENTINEL, dtype=torch.uint8, device="cuda"),
            "het": torch.full(shape + (d.nbin,), zf.FILL, dtype=torch.int32, device="cuda"),
            "runs": torch.full(shape + (32,), zf.FILL, dtype=torch.int32, device="cuda")}
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = lambda k: bufs[k].data_ptr() if k in d.want else None  # noqa: E731
    rc = lib.phk_simulate(0, K, P.data_ptr(), P.stride(0), P.stride(1) if d.per_row else 0, d.B, d.S, d.n_rep, d.L, ctypes.c_uint64(d.key),
                          ctypes.c_int64(d.seq0), None if mask is None else mask.data_ptr(), 0 if mask is None else mask.stride(0), ptr("obs"),
                          ptr("paths"), d.stride, d.bin, ptr("het"), ptr("runs"), flags.data_ptr(), None)
    assert rc == _lib.PHK_OK, lib.phk_last_error()
    torch.cuda.synchronize()
    out = {k: bufs[k].cpu().numpy() for k in zf.OUTS}
    out["flags"] = int(flags.item())
    return out


def _simulate_draw(seed, record=True):
    import torch

    t0 = time.perf_counter()
    d = zf.draw(seed)
    zf.oracle(d)
    P = torch.as_tensor(np.stack(list(d.pp), -2)).cuda().contiguous()  # [B, S or 1, 7, K]
    assert P.shape == (d.B, d.S if d.per_row else 1, 7, d.K)
    mask = _mask_tensor(d)
    got = raw_call(d, P, mask)
    msg = zf.compare(d, got)
    print(f"fuzz simulate {zf.describe(d)}: {'equal' if msg is None else msg}")
    assert msg is None, msg
    again = raw_call(d, P, mask)  # a repeat call: the same bytes
    for k in zf.OUTS + ("flags",):
        assert np.array_equal(got[k], again[k]), k
    if record:
        STATS.append(dict(entries=sum(got[k].size for k in d.want), flag=got["flags"] & 1, time=time.perf_counter() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_simulate_random_shapes(seed):
    _simulate_draw(seed)


@pytest.mark.gpu
def test_regression_draws():
    """every pinned draw, whatever the number of seeds run (a loop: the table may be empty, and an empty parameter list skips)"""
    for name in sorted(REGRESSIONS):
        _simulate_draw(REGRESSIONS[name], record=False)


@pytest.mark.gpu
def test_simulate_rows_with_seventy_replicates():
    """the public layer past one workgroup per block: two models, ragged contigs, 70 replicates per row (three rows: 210
    sequences share a block), equal to the oracle at every entry"""
    import phlash_amd
    from test_simulate import _public_blocks
    from phlash_amd.size_history import DemographicModel

    g = np.random.default_rng(18)
    contigs = [(g.random((2, 60)) < 0.05).astype(np.int8), (g.random((1, 41)) < 0.05).astype(np.int8)]
    for c in contigs:
        c.flat[g.integers(0, c.size, 6)] = -1
    contigs[0][1, 20:37] = -1
    dms = [DemographicModel.default("16*1", 5e-4, 5e-4), DemographicModel.default("16*1", 7e-4, 4e-4)]
    R, seed = 70, (5 << 32) | 99
    out = phlash_amd.simulate_rows(dms, contigs, n_rep=R, seed=seed, paths=True)
    blocks = _public_blocks(dms)
    N, row0 = 3, 0
    for c, obs, paths in zip(contigs, out.obs, out.paths):
        n, length = c.shape
        assert obs.shape == (2, n, R, length) and paths.shape == obs.shape
        for b in range(2):
            for s in range(n):
                ref = sim.simulate_paths(blocks[b], length, np.full(R, b * N + row0 + s), np.arange(R), seed, margins=False)
                assert not ref["flag"]
                assert np.array_equal(paths[b, s].cpu().numpy(), ref["paths"]), (b, s)
                assert np.array_equal(obs[b, s].cpu().numpy(), sim.lay_mask(ref["codes"], c[s])), (b, s)
        row0 += n
