"""HIP-event time of a sampled-tract-spectrum call (phk_sample_tracts, cover on and off) against a path-sampling call
(phk_sample_paths) with the same arguments in the same process, K = 16, float32 kernels (not run by bench.py).

Shapes: (b) 100 models x 20 rows x 100,000 windows; (c) the reference's production shape, 500 x 5 x 100,000; both at 5 % hets.
n_samples = 1 and 8 against the path call, n_samples = 64 for the new call alone (its paths would be 12.8 GB).  Before it reports
a shape the script checks the new call against ``path_tracts`` of the stored paths of the first particles (equal at every entry)
and its ll against the path call's (bitwise), and prints one JSON line per shape and n_samples with the library's sha256.

    python scripts/sample_tracts_timing.py [--shapes bc] [--samples 1,8,64] [--reps 5]
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"b": (100, 20, 100_000, 0.05), "c": (500, 5, 100_000, 0.05)}
EDGES, MIN_LEN, BIN = (10, 100, 1000), 100, 100
PATHS_UP_TO = 8  # n_samples above this: the new call alone


def rows(S, L, het, seed):
    g = np.random.default_rng(seed)
    d = (g.random((S, L), dtype=np.float32) < het).astype(np.int8)
    d.flat[g.integers(0, d.size, size=int(0.01 * d.size))] = -1
    d[:, 0] = 1
    return d


def timed(fns, reps):
    """medians (ms) of ``reps`` alternating calls of every function after one warm-up call of each"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bc")
    ap.add_argument("--samples", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from phlash_amd import _lib, path_tracts
    from phlash_amd.engine import HipEngine
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population

    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    member = np.arange(16) < 11  # the set: the eleven youngest states (scripts/moments_timing.py's tract weights)
    mask = torch.tensor([sum(1 << k for k in range(16) if member[k])], dtype=torch.int64, device="cuda")
    for key in args.shapes:
        B, S, L, het = SHAPES[key]
        data = rows(S, L, het, seed=7)
        tmpl, x = particle_population(16, B, seed=1, sigma=0.25)
        P = PSMCParams.from_dm(tmpl.from_flat(x).to_dm()).stack()[:, None].cuda()  # [B, 1, 7, K] float64
        eng = HipEngine(16, data, double_precision=False)
        inds = torch.arange(S, device="cuda")
        # the check, on the first two particles: equal to path_tracts of the stored paths at every entry, ll bitwise
        ll, stats, cover = eng.sample_tracts(P[:2], inds, mask, n_samples=2, seed=3, edges=EDGES, min_len=MIN_LEN, bin=BIN)
        ll2, paths = eng.sample_paths(P[:2], inds, n_samples=2, seed=3)
        assert not eng.underflow_risk()
        want = path_tracts(paths, member, edges=EDGES, min_len=MIN_LEN, bin=BIN)
        assert torch.equal(stats[..., :4], want.counts) and torch.equal(stats[..., 4:], want.hist) and torch.equal(cover, want.cover)
        assert torch.equal(ll, ll2)
        tracts_per_row = float(stats[..., 1].double().mean())
        check = (f"stats and cover equal path_tracts of the stored paths on 2 particles x {S} rows x 2 samples ({tracts_per_row:.0f} tracts per "
                 f"path, {float(cover.sum()) / float(stats[..., 0].sum()):.3f} of the sites inside lie in a tract >= {MIN_LEN}); ll bitwise phk_sample_paths'")
        del paths, want, stats, cover
        for n in (int(v) for v in args.samples.split(",")):
            fns = [lambda: eng.sample_tracts(P, inds, mask, n_samples=n, seed=3, edges=EDGES, min_len=MIN_LEN, bin=BIN),
                   lambda: eng.sample_tracts(P, inds, mask, n_samples=n, seed=3, edges=EDGES)]
            if n <= PATHS_UP_TO:
                fns.append(lambda: eng.sample_paths(P, inds, n_samples=n, seed=3))
            t = timed(fns, args.reps)
            assert not eng.underflow_risk()
            rec = {"shape": key, "B": B, "S": S, "L": L, "het": het, "n_samples": n, "tracts_cover_ms": round(t[0], 3), "tracts_ms": round(t[1], 3)}
            if n <= PATHS_UP_TO:
                rec.update(paths_ms=round(t[2], 3), ratio_cover_to_paths=round(t[0] / t[2], 3), ratio_to_paths=round(t[1] / t[2], 3),
                           path_bytes=B * S * n * L)
            rec.update(plan=eng.get_plan(), check=check, lib_sha256=sha)
            print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
