"""The hand-written block run of the K = 16 float32 sweeps (csrc/sweep_run_k16r2.inc, scripts/gen_sweep_asm.py) without the vector
instructions its result does not need: the `x + 0` scan seeds are read from their source registers, and an all-hom block keeps
suf(v.*w) of seven of its eight sites between its two passes (one of them in eight floats of the thread's LDS slice).  Every
instruction that is left has the C++ body's operands in the C++ body's order, so run on / run off (``phk_set_asm_run``) must give
the SAME BITS: log-likelihoods and every gradient row.

GPU cases: one per (particles x chunks, plan, kind of rows); each walks the lengths and warm-ups below.  33 and 40 particles put
one and two observation rows into a wave (3 particles x 3 chunks put three: such a wave keeps the C++ loop whatever is asked);
2,600 sites give the segment sweep several units -- a unit's first and last block -- and cross the fold of the partial sums; a
warm-up of 8 sites ends on a block boundary, one of 500 inside a block.  Rows:
    hom        no het, no missing site: every block takes the all-hom body, i.e. the parked and the kept vectors
    mix        1 % hets + 1 % missing sites
    het8       one het per third block, at each of the eight positions of a block in turn (each row starts at another position)
    missruns   runs of 1 .. 40 missing sites, at every alignment to the blocks
    massless   0.2 % hets, and particles some of whose states carry no mass at all (pi = b = v = 0 there: a whole lane's eight states, the
               other lane's, states at both ends, the two in the middle, all but one), so that the scans' totals and carries -- the seeds that are
               no longer added to zero -- are exact zeros.  (No more hets than that: every het multiplies the gradient of the particle
               whose upper eight states are dead by about ten in the float64 oracle, 1e36 at 1 % hets and 2,600 sites, which float32
               cannot hold in either body; at 0.2 % the oracle's largest entry is below 1e8.  One particle in eight has ONE state alive, state
               5: a lone live state at the top of the time axis has a gradient float32 cannot hold at all, 1e113 after 1,040 sites.
               Such a particle used to turn its neighbours in the 16-lane row into NaN, in both bodies alike -- inf times the 0 of
               a lane mask; tests/test_massless_fuzz.py holds that case, and these models against the oracle.))

The CPU test holds the generator's own report: the vector instructions of one all-hom trip, no s_nop, the slice's size."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import psmc_numpy as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(3, 2), (3, 3), (33, 2), (33, 3), (40, 2), (40, 3)]
LENGTHS = (520, 1040, 2600)
WARMUPS = (0, 8, 500)
PLANS = ("serial", "hybrid", "segmented")
ROWS = ("hom", "mix", "het8", "missruns", "massless")


def test_generator_report_holds_the_counts():
    """670 vector instructions per all-hom trip before; 28 identity adds and half of the 22 of the two recomputed sites are gone at
    least: <= 631.  No s_nop in either body.  Two 256-thread workgroups per CU: at most 80 floats of LDS per thread."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_sweep_asm.py"), "--report"], check=True,
                         capture_output=True, text=True).stdout
    print(out)
    counts = {}
    for kind, rest in re.findall(r"^(all-hom|mixed) block: (.*)$", out, re.M):
        counts[kind] = {k: int(v) for k, v in re.findall(r"([A-Za-z_]+) (\d+)", rest)}
    assert set(counts) == {"all-hom", "mixed"}, out
    assert counts["all-hom"]["vector"] <= 631
    assert counts["all-hom"]["s_nop"] == 0 and counts["mixed"]["s_nop"] == 0
    assert counts["mixed"]["vector"] <= 715  # (the mixed trip before)
    floats = int(re.search(r"LDS slice: (\d+) floats per thread", out).group(1))
    assert floats <= 80
    assert (floats // 4) % 2 == 1 and floats % 4 == 0  # odd in 16-byte units: the lanes of a ds_read_b128 fall on different banks


_PARAMS = {}


def _params(B, S, massless):
    """B particles around the default model, K = 16 -> [B, S, 7, 16] (rows b, d, u, v, emis0, emis1, pi; computed once per shape)"""
    key = (B, S, massless)
    if key not in _PARAMS:
        rng = np.random.default_rng(100 * B + S)
        pat = "14*1+1*2"
        x0 = o.particle_from_linear(pat, 1e-4, 15.0, np.ones(len(o.parse_pattern(pat))), 1e-2, 1e-2)
        out = np.zeros((B, S, 7, 16))
        for b in range(B):
            x = x0 + 0.3 * rng.normal(size=x0.shape) * (b > 0)
            out[b, :] = o.from_dm(o.particle_to_dm(x, pat, 1e-2)).stack()
            # states without mass: nothing starts there (pi) and nothing arrives there (b, v: the off-diagonal columns)
            dead = {1: range(0, 8), 2: range(8, 16), 3: (0, 1, 14, 15), 4: [k for k in range(16) if k != 5],
                    5: (7, 8)}.get(b % 8, ()) if massless else ()
            for k in dead:
                out[b, :, [0, 3, 6], k] = 0.0
        out.setflags(write=False)
        _PARAMS[key] = out
    return _PARAMS[key]


_DATA = {}


def _rows(kind, S, L):
    if (kind, S, L) in _DATA:
        return _DATA[(kind, S, L)]
    rng = np.random.default_rng(1000 * ROWS.index(kind) + 7 * S + L)
    data = np.zeros((S, L), np.int8)
    if kind in ("mix", "massless"):
        data[:] = rng.uniform(size=(S, L)) < (0.01 if kind == "mix" else 0.002)
    if kind == "mix":
        data.flat[rng.integers(0, data.size, data.size // 100)] = -1
    if kind == "het8":
        for s in range(S):
            for k in range((L - 16) // 24):
                data[s, 24 * k + 8 + (k + 3 * s) % 8] = 1
    if kind == "missruns":
        for s in range(S):
            at = 9 + 3 * s
            for n, run in enumerate((1, 2, 5, 8, 9, 17, 40, 3, 16, 7)):
                if at + run >= L:
                    break
                data[s, at:at + run] = -1
                at += run + 8 * (2 + n % 3) + 1  # (the next run starts one position further into its block)
    data[:, 0] = np.maximum(data[:, 0], 0)
    data.setflags(write=False)
    _DATA[(kind, S, L)] = data
    return data


def _run(eng, p, i, W):
    import torch

    ll, g = eng.run(p, i, warmup=W, grad=True)
    torch.cuda.synchronize()
    return ll.cpu().numpy(), g.cpu().numpy()


def _set_plan(eng, plan, B):
    eng.set_autotune(False)
    eng.set_rescale_interval(4)
    if plan == "serial":
        eng.set_plan(0, R=2, T=8, R_forward=1, R_scan=0)
    elif plan == "segmented":
        eng.set_plan(1, R=2, T=8, R_forward=16, R_scan=16)
    else:  # serial sweep of the first chunk's sequences beside the segment sweep of the rest
        eng.install_plan({"segmented": 0, "R": 2, "T": 8, "R_forward": 1, "hybrid_first": B, "R_segment_sweep": 2, "R_scan": 16})


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_run_on_equals_run_off(shape, plan, rows):
    torch = pytest.importorskip("torch")
    from phlash_amd.engine import HipEngine

    B, S = shape
    p = torch.tensor(_params(B, S, rows == "massless"), device="cuda")
    i = torch.arange(S, dtype=torch.int64, device="cuda")
    for L in LENGTHS:
        eng = HipEngine(16, _rows(rows, S, L), double_precision=False)
        _set_plan(eng, plan, B)
        for W in WARMUPS:
            assert eng.get_asm_run()
            ll_on, g_on = _run(eng, p, i, W)
            eng.set_asm_run(False)
            assert not eng.get_asm_run()
            ll_off, g_off = _run(eng, p, i, W)
            eng.set_asm_run(True)
            what = f"L = {L}, W = {W}"
            if plan == "hybrid":  # (the plan of the run just made)
                assert eng.get_plan().get("hybrid_first") == B, what
            else:
                assert eng.get_plan()["segmented"] == (plan == "segmented"), what
            assert np.isfinite(ll_off).all() and np.isfinite(g_off).all() and np.abs(g_off).max() > 0, what
            assert g_on.shape == (B, S, 7, 16) and g_on.dtype == g_off.dtype and ll_on.dtype == ll_off.dtype, what
            assert ll_on.tobytes() == ll_off.tobytes(), what
            bits = f"u{g_on.itemsize}"
            bad = g_on.view(bits) != g_off.view(bits)  # bit for bit: the sign of a zero included
            assert not bad.any(), f"{what}: {int(bad.sum())} gradient entries differ, rows {sorted(set(np.nonzero(bad)[2].tolist()))}"
