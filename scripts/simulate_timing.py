"""HIP-event time of posterior predictive simulation (phk_simulate), K = 16 (not run by bench.py).

(a) obs only, 100 models x 20 rows x 1 replicate x 100,000 windows under the rows' own masks, against phk_sample_paths
    (float32 kernels, n_samples = 1) on a 100 x 20 x 100,000 handle: the two calls alternate in one process after a warm-up
    call of each, medians of ``--reps`` calls;
(b) het + runs only (bin = 100), 100 x 5 x 100 x 100,000: no row is stored;
(c) phlash_amd.synth.simulate_chunks, 2,000 rows x 100,000 sites, on the host of the same box, once, for the record.
Before it times a shape the script checks one sequence of the call against the float64 statement of tests/simulate_oracle.py
(every site of obs for (a); het and runs for (b)).  One JSON line per shape, the static instruction count of the site loop
(scripts/loop_report.py, when the object file is there) and the library's sha256, to stdout and to ``--out``.

    python scripts/simulate_timing.py [--shapes abc] [--reps 5] [--out profiles/simulate_timing.txt]
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SEED = 2024
L = 100_000


def rows(S, n, het, seed):
    g = np.random.default_rng(seed)
    d = (g.random((S, n), dtype=np.float32) < het).astype(np.int8)
    d.flat[g.integers(0, d.size, size=int(0.01 * d.size))] = -1
    d[:, 0] = 1
    return d


def timed(fns, reps):
    """medians (ms) of ``reps`` alternating calls of the functions after one warm-up call of each"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for f, t in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in ts]


def static_count():
    obj = os.path.join(ROOT, "phlash_amd", "csrc", "build", "launch_simulate.o")
    if not os.path.exists(obj):
        return None
    from loop_report import kernel_loops

    out = {}
    for name, k in kernel_loops(obj, "simulate_kernel").items():
        tag = {"ILb1ELb1E": "rows+stats", "ILb1ELb0E": "rows", "ILb0ELb1E": "stats"}[[t for t in ("ILb1ELb1E", "ILb1ELb0E", "ILb0ELb1E") if t in name][0]]
        big = max(k["loops"], key=lambda r: r["n"])  # the 16-site block loop
        out[tag] = {"per_block": big["n"], "per_site": round(big["n"] / 16, 1), "valu": big["valu"], "lds": big["lds"], "global": big["global"],
                    "scratch": k["scratch"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simulate_timing.txt"))
    args = ap.parse_args()
    from phlash_amd import _lib
    from phlash_amd.engine import HipEngine
    from phlash_amd.params import PSMCParams
    from phlash_amd.simulate import simulate
    from phlash_amd.synth import particle_population, simulate_chunks
    import simulate_oracle as so
    from oracle import psmc_numpy as pn

    lines = [f"# scripts/simulate_timing.py --shapes {args.shapes} --reps {args.reps}: K = 16, HIP-event medians of alternating calls in one process"]

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    emit({"lib_sha256": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), "static_site_loop": static_count()})

    def population(B):
        tmpl, x = particle_population(16, B, seed=1, sigma=0.25)
        pp = PSMCParams.from_dm(tmpl.from_flat(x).to_dm())
        return pp, pp.stack()[:, None].cuda()  # [B, 1, 7, K] float64

    def block(pp, b):
        return pn.PP(*(getattr(pp, name)[b].numpy() for name in pn.PP._fields))

    if "a" in args.shapes:
        B, S = 100, 20
        data = rows(S, L, 0.02, seed=7)
        pp, P = population(B)
        mask = torch.as_tensor(data).cuda()
        out = simulate(P, L, n_rep=1, seed=SEED, mask=mask)
        b, s = B - 1, S - 1
        ref = so.simulate(block(pp, b), 2000, b * S + s, 1, SEED, mask_row=data[s])
        assert int(out.flags.item()) == 0 and np.array_equal(out.obs[b, s, :, :2000].cpu().numpy(), ref["obs"])
        del out
        eng = HipEngine(16, data, double_precision=False)
        inds = torch.arange(S, device="cuda")
        t_sim, t_smp = timed([lambda: simulate(P, L, n_rep=1, seed=SEED, mask=mask), lambda: eng.sample_paths(P, inds, 0, n_samples=1, seed=SEED)], args.reps)
        emit({"shape": "a", "B": B, "S": S, "n_rep": 1, "L": L, "outputs": "obs", "simulate_ms": round(t_sim, 3), "sample_paths_f32_ms": round(t_smp, 3),
              "ratio": round(t_sim / t_smp, 3), "check": "sequence (99, 19), sites 0..1999 of obs equal to the float64 statement"})
        del eng
        torch.cuda.empty_cache()
    if "b" in args.shapes:
        B, S, R = 100, 5, 100
        data = rows(S, L, 0.02, seed=8)
        pp, P = population(B)
        mask = torch.as_tensor(data).cuda()
        out = simulate(P, L, n_rep=R, seed=SEED, mask=mask, obs=False, bin=100, runs=True)
        b, s = B - 1, S - 1
        short = simulate(P[b:], 3000, n_rep=2, seed=SEED, mask=mask, seq0=b * S, obs=False, bin=100, runs=True)
        ref = so.simulate(block(pp, b), 3000, b * S + s, 2, SEED, mask_row=data[s], bin=100)
        assert int(out.flags.item()) == 0 and np.array_equal(short.het[0, s].cpu().numpy(), ref["het"]) and np.array_equal(short.runs[0, s].cpu().numpy(), ref["runs"])
        assert np.array_equal(out.het[b, s, :2, :30].cpu().numpy(), ref["het"])
        del out, short
        (t_sim,) = timed([lambda: simulate(P, L, n_rep=R, seed=SEED, mask=mask, obs=False, bin=100, runs=True)], args.reps)
        emit({"shape": "b", "B": B, "S": S, "n_rep": R, "L": L, "outputs": "het(bin=100)+runs", "simulate_ms": round(t_sim, 3),
              "site_draws_per_s": round(B * S * R * L / (t_sim * 1e-3), 0), "check": "sequence (99, 4), 2 replicates, 3,000 sites: het and runs equal to the float64 statement"})
        torch.cuda.empty_cache()
    if "c" in args.shapes:
        t0 = time.perf_counter()
        simulate_chunks(16, 2000, L, seed=1)
        emit({"shape": "c", "what": "synth.simulate_chunks on the host", "rows": 2000, "L": L, "seconds": round(time.perf_counter() - t0, 2)})
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
