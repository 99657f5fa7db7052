"""HIP-event time of a path-sampling call (phk_sample_paths) against a Viterbi call (phk_viterbi) on the same inputs, K = 16,
float32 kernels (not run by bench.py).

Shapes (those of scripts/viterbi_timing.py): (b) 100 models x 20 rows x 100,000 windows; (c) the reference's production
shape, 500 x 5 x 100,000 at 5 % hets; each with n_samples = 1 and 8.  The two calls alternate in one process, after a warm-up
call of each; the medians of ``--reps`` calls are reported.  Before it reports a shape the script checks the sampling call
against the float64 oracle of tests/sampling_oracle.py on two (model, row) pairs by the float32 rule of
tests/test_path_sampling.py: every path equals the oracle's up to a draw that float32 cannot decide.  One JSON line per
shape and n_samples with the library's sha256.

    python scripts/sample_timing.py [--shapes bc] [--reps 5]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"b": (100, 20, 100_000, 0.02), "c": (500, 5, 100_000, 0.05)}
SEED = 2024


def rows(S, L, het, seed):
    g = np.random.default_rng(seed)
    d = (g.random((S, L), dtype=np.float32) < het).astype(np.int8)
    d.flat[g.integers(0, d.size, size=int(0.01 * d.size))] = -1
    d[:, 0] = 1
    return d


def timed_pair(f, g, reps):
    """medians (ms) of ``reps`` alternating calls of f and g after one warm-up call of each"""
    f()
    g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        for fn, ts in ((f, tf), (g, tg)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    return float(np.median(tf)), float(np.median(tg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bc")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from phlash_amd import _lib
    from phlash_amd.engine import HipEngine
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population
    import sampling_oracle as so
    from decode_fuzz import F32_GAMMA_BAR
    from oracle import psmc_numpy as pn

    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    for key in args.shapes:
        B, S, L, het = SHAPES[key]
        data = rows(S, L, het, seed=7)
        tmpl, x = particle_population(16, B, seed=1, sigma=0.25)
        pp = PSMCParams.from_dm(tmpl.from_flat(x).to_dm())
        P = pp.stack()[:, None].cuda()  # [B, 1, 7, K] float64
        eng = HipEngine(16, data, double_precision=False)
        inds = torch.arange(S, device="cuda")
        ll, paths = eng.sample_paths(P, inds, 0, n_samples=2, seed=SEED)
        assert not eng.underflow_risk()
        assert torch.isfinite(ll).all() and int(paths.max()) < 16
        diverged = 0
        for b, s in ((0, 0), (B - 1, S - 1)):
            q = pn.PP(*(getattr(pp, name)[b].numpy() for name in pn.PP._fields))
            alpha = so.forward(q, data[s])
            ref, margins = so.sample(q, data[s], 0, b * S + s, 2, SEED, bits24=True, alpha=alpha)
            n, bad = so.f32_divergences(q, data[s], 0, ref, margins, paths[b, s].cpu().numpy(), F32_GAMMA_BAR, alpha64=alpha)
            assert not bad, bad
            diverged += n
        check = f"2 sequences x 2 samples vs the float64 oracle: {diverged} of 4 paths diverged, each at a draw float32 cannot decide"
        del paths
        for n_samples in (1, 8):
            t_smp, t_vit = timed_pair(lambda: eng.sample_paths(P, inds, 0, n_samples=n_samples, seed=SEED),
                                      lambda: eng.viterbi(P, inds, 0), args.reps)
            print(json.dumps({"shape": key, "B": B, "S": S, "L": L, "het": het, "n_samples": n_samples, "sample_ms": round(t_smp, 3),
                              "ms_per_sample": round(t_smp / n_samples, 3), "viterbi_ms": round(t_vit, 3),
                              "ratio": round(t_smp / t_vit, 3), "check": check, "lib_sha256": sha}), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
