"""Seeded random draws for posterior predictive simulation (``phk_simulate``), the oracle of a draw and the comparator that
holds the buffers a call leaves behind against it.  Test infrastructure only, CPU only; used by tests/test_simulate_fuzz.py
(the GPU tests and the CPU self-tests share the comparator).

A draw holds everything a call depends on, from a random stream of its own: K, B x S, one block per particle or per
(particle, row), the replicates per row, L, the models (a sigma = 0.25 population with theta and rho scaled, on a share of the
draws with a state whose transition row has no mass, a state whose emission rows have none, or pi on the last state), the
mask and how it is stored, a 64-bit seed, seq0, which outputs are asked for, the bin and the row stride.  K, the replicates
and L are stratified by seed; L is stepped down its list until the oracle's Python loop has at most MAX_STEPS site steps.

Reference: simulate_oracle.simulate_paths / lay_mask / statistics.  The kernel runs the same IEEE float64 operations in the
same order, so the comparison is equality at every entry: no tolerance, no exemption by margin (the oracle's margin at the
first mismatch is printed, to tell a draw next to a boundary from a wrong index).  Also held: flags & 1 is the oracle's flag,
bytes at or past L of every row keep the sentinel, buffers that were not asked for keep their fill.
"""

from __future__ import annotations

import functools
import types

import numpy as np

import simulate_oracle as sim
from oracle import psmc_numpy as pn

KS = [2, 3, 4, 5, 7, 8, 12, 16, 17, 31, 32, 33, 48, 63, 64]
NREPS = [1, 3, 7, 21, 22, 63, 64, 65, 70, 129]
LS = [1, 2, 15, 16, 17, 31, 32, 33, 48, 100, 257]
SCALES = [0.1, 1.0, 10.0]
SEQ0S = [0, 5, 2 ** 32 + 3, 2 ** 40]
MASKS = ("none", "holes", "row_missing", "lastbin")
STORES = ("aligned", "offset", "tight")  # pointer and stride multiples of 16 / a view one byte into its buffer / stride L
SPECIALS = ("none", "none", "none", "dead_state", "dead_emission", "pi_last")
OUTS = ("obs", "paths", "het", "runs")
NT = 64  # lanes of a workgroup: one sequence each
MAX_STEPS = 40_000
SENTINEL = 0x55
FILL = -7  # of the statistic buffers


def ceil16(n):
    return -(-n // 16) * 16


def _blocks(K, n, seed, scale):
    """n valid models with K states: a sigma = 0.25 particle population with theta and rho scaled -> pn.PP, fields [n, K]"""
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population

    if K < 3:  # (the population's pattern ties the last two states and needs three): random sizes on the default grid
        g = np.random.default_rng(seed)
        dm = pn.default_dm(f"{K}*1", 1e-2 * scale, 1e-2 * scale)
        pps = [pn.from_dm(pn.DM(dm.t, np.exp(0.5 * g.standard_normal(K)), 1e-2 * scale * np.exp(0.5 * g.standard_normal()),
                                1e-2 * scale * np.exp(0.5 * g.standard_normal()))) for _ in range(n)]
        return pn.PP(*(np.stack([np.asarray(getattr(q, f), float) for q in pps]) for f in pn.PP._fields))
    tmpl, x = particle_population(K, n, seed=seed, theta=1e-2 * scale, sigma=0.25)
    pp = PSMCParams.from_dm(tmpl.from_flat(x).to_dm())
    return pn.PP(*(np.array(a.numpy(), float).reshape(n, K) for a in pp))


class Draw(types.SimpleNamespace):
    def block(self, b, s):
        return pn.PP(*(a[b, s if self.per_row else 0] for a in self.pp))

    @property
    def per_block(self):
        """sequences that share a parameter block: one workgroup takes 64 of them"""
        return self.n_rep if self.per_row else self.S * self.n_rep

    @property
    def nbin(self):
        return -(-self.L // self.bin)


def describe(d):
    return (f"seed={d.seed} K={d.K} B={d.B} S={d.S} {'rows' if d.per_row else 'bcast'} n_rep={d.n_rep} L={d.L} scale={d.scale} "
            f"special={d.special} mask={d.mask_kind}/{d.store} key={d.key:#x} seq0={d.seq0} want={'+'.join(d.want)} bin={d.bin} "
            f"stride={d.stride}")


@functools.lru_cache(maxsize=None)
def draw(seed):
    rng = np.random.default_rng([30_000 + seed, 0])
    d = Draw(seed=seed)
    d.K = K = KS[seed % 15]
    d.n_rep = NREPS[(seed + seed // 15) % 10]
    d.B, d.S = int(rng.integers(1, 4)), int(rng.integers(1, 5))
    d.per_row = bool(rng.integers(2)) and d.S > 1  # (one row: the call has no row stride to tell the layouts apart)
    li = (7 * seed + seed // 11) % 11
    while li > 0 and d.B * d.S * d.n_rep * LS[li] > MAX_STEPS:
        li -= 1
    d.L = L = LS[li]
    d.scale = SCALES[int(rng.integers(3))]
    Sp = d.S if d.per_row else 1
    pp = _blocks(K, d.B * Sp, 200 + seed, d.scale)
    pp = pn.PP(*(a.reshape(d.B, Sp, K).copy() for a in pp))
    d.special = SPECIALS[int(rng.integers(len(SPECIALS)))]
    d.dead = None
    if d.special == "dead_state" and K < 3:
        d.special = "none"  # (no interior state)
    if d.special == "dead_state":  # the last particle: interior state i has no mass in its row and is reachable from both sides
        d.dead = i = int(rng.integers(1, K - 1))
        pp.b[-1, :, :i] = 0.0
        pp.d[-1, :, i] = 0.0
        pp.u[-1, :, i] = 0.0
    elif d.special == "dead_emission":
        d.dead = i = int(rng.integers(0, K))
        pp.emis0[-1, :, i] = 0.0
        pp.emis1[-1, :, i] = 0.0
    elif d.special == "pi_last":
        pp.pi[-1, :, :] = 0.0
        pp.pi[-1, :, K - 1] = 1.0
    d.pp = pp
    d.mask_kind = MASKS[int(rng.integers(len(MASKS)))]
    d.store = STORES[int(rng.integers(len(STORES)))]
    if d.store == "tight" and L % 16 == 0:
        d.store = "offset"  # (a stride of L would be aligned)
    d.bin = int([1, 7, 16, 100, L, L + 5][int(rng.integers(6))])
    d.mask = None
    if d.mask_kind != "none":
        m = np.zeros((d.S, L), np.int8)
        if d.mask_kind == "holes":  # isolated missing sites in every row and one run
            for s in range(d.S):
                m[s, rng.integers(0, L, size=max(1, L // 12))] = -1
            a = int(rng.integers(0, L))
            m[int(rng.integers(d.S)), a : a + max(1, L // 4)] = -1
        elif d.mask_kind == "row_missing":
            m[int(rng.integers(d.S))] = -1
        else:
            m[int(rng.integers(d.S)), d.bin * ((L - 1) // d.bin) :] = -1
        d.mask = m
    d.key = int(rng.integers(0, 2 ** 32))
    if rng.integers(2):
        d.key |= int(rng.integers(1, 2 ** 32)) << 32
    d.seq0 = SEQ0S[int(rng.integers(4))]
    bits = int(rng.integers(1, 16))
    d.want = tuple(o for k, o in enumerate(OUTS) if bits >> k & 1)
    d.stride = ceil16(L) + 16 * int(rng.integers(2))
    return d


# ------------------------------------------------------------------------------------------------- oracle of a draw
def oracle(d, margins=False):
    """-> dict(paths uint8 [B, S, n_rep, L], codes int8 likewise (unmasked), obs (masked), het int32 [B, S, n_rep, nbin], runs
    int32 [B, S, n_rep, 32], flag); kept on the draw (``margins=True``: computed afresh with m_path and m_obs, for a message)"""
    if not margins and getattr(d, "_oracle", None) is not None:
        return d._oracle
    shape = (d.B, d.S, d.n_rep, d.L)
    out = dict(paths=np.empty(shape, np.uint8), codes=np.empty(shape, np.int8), flag=False)
    if margins:
        out.update(m_path=np.empty(shape), m_obs=np.empty(shape))
    for b in range(d.B):
        for s in range(d.S):
            o = sim.simulate_paths(d.block(b, s), d.L, np.full(d.n_rep, d.seq0 + b * d.S + s, dtype=np.uint64), np.arange(d.n_rep), d.key,
                                   margins=margins)
            out["paths"][b, s], out["codes"][b, s] = o["paths"], o["codes"]
            out["flag"] = out["flag"] or bool(o["flag"])
            if margins:
                out["m_path"][b, s], out["m_obs"][b, s] = o["m_path"], o["m_obs"]
    out["obs"] = lay(out["codes"], d.mask)
    out["het"], out["runs"] = stats(out["obs"], d.bin)
    if not margins:
        d._oracle = out
    return out


def lay(codes, mask):
    """the mask of row s over codes [B, S, n_rep, L]"""
    if mask is None:
        return codes.copy()
    return np.stack([sim.lay_mask(codes[:, s], mask[s]) for s in range(codes.shape[1])], 1)


def stats(obs, bin, statistics=sim.statistics):
    B, S, R, L = obs.shape
    het, runs = statistics(obs.reshape(-1, L), bin)
    return het.reshape(B, S, R, -1), runs.reshape(B, S, R, 32)


def buffers(d, obs, paths, het, runs, flag):
    """what a call of draw ``d`` leaves in its four buffers and its flag word if its outputs are these: rows at the draw's
    stride over the sentinel, the buffers that were not asked for at their fill"""
    shape = (d.B, d.S, d.n_rep)
    out = {"obs": np.full(shape + (d.stride,), SENTINEL, np.int8), "paths": np.full(shape + (d.stride,), SENTINEL, np.uint8),
           "het": np.full(shape + (d.nbin,), FILL, np.int32), "runs": np.full(shape + (32,), FILL, np.int32), "flags": int(bool(flag))}
    for k, v in (("obs", obs), ("paths", paths)):
        if k in d.want:
            out[k][..., : d.L] = v
    for k, v in (("het", het), ("runs", runs)):
        if k in d.want:
            out[k][:] = v
    return out


def oracle_candidate(d):
    o = oracle(d)
    return buffers(d, o["obs"], o["paths"], o["het"], o["runs"], o["flag"])


# ------------------------------------------------------------------------------------------------- comparator
def compare(d, got):
    """-> None, or the first difference between the buffers ``got`` (as ``buffers`` lays them out) and the oracle's"""
    want = oracle_candidate(d)
    for k in OUTS:
        g, w = np.asarray(got[k]), want[k]
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"{k}: shape / type {g.shape} {g.dtype}, expected {w.shape} {w.dtype}"
        if k not in d.want:
            if not np.array_equal(g, w):
                return f"{k} was not asked for and its buffer changed"
            continue
        if k in ("obs", "paths") and not (g[..., d.L :] == w[..., d.L :]).all():
            i = tuple(np.argwhere(g[..., d.L :] != w[..., d.L :])[0])
            return f"{k}: a byte at or past L = {d.L} was written (sequence {i[:3]}, byte {d.L + i[3]})"
        bad = np.argwhere(g != w)
        if len(bad):
            i = tuple(bad[0])
            m = ""
            if k in ("obs", "paths"):
                mm = oracle(d, margins=True)["m_obs" if k == "obs" else "m_path"][i]
                m = f", the oracle's margin there {mm:.3e}"
            return f"{k}: {len(bad)} entries differ, first at {i}: got {g[i]}, oracle {w[i]}{m}"
    if (int(got["flags"]) & 1) != want["flags"]:
        return f"flags & 1 is {int(got['flags']) & 1}, the oracle's flag is {want['flags']}"
    return None
