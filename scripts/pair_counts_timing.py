"""HIP-event time of a pair-count call (``phk_pair_counts``) against a transition-posterior call (``changes`` and ``arrivals``,
bin = 100) and a posterior-decoding call (marginals, bin = 100) on the same inputs (not run by bench.py).

Shapes, K = 16 float32 at 5 % hets: (b) 100 models x 20 rows x 100,000 windows; (c) the reference's production shape,
500 x 5 x 100,000.  One line each at a reduced batch for the generic path: (k) K = 64 float32 and (d) K = 16 float64, 20 x 5 x
100,000, where a call makes several launches of the sweep.  Before it reports a shape the script checks ``counts`` against the
float64 dense oracle of tests/pair_count_oracle.py on two (model, row) pairs, and prints one JSON line per shape with the
library's sha256.  The plain-HIP template at K = 16 float32 is timed by running the script on a library built with
``AB_ALSO=launch_pairs scripts/ab_build.sh plain f32 16 -DPHK_PAIRS_MFMA=0`` (``PHK_LIB=<path>``).

    python scripts/pair_counts_timing.py [--shapes bckd] [--reps 5]
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

# key: (K, float64?, B, S, L, het)
SHAPES = {"b": (16, False, 100, 20, 100_000, 0.05), "c": (16, False, 500, 5, 100_000, 0.05),
          "k": (64, False, 20, 5, 100_000, 0.05), "d": (16, True, 20, 5, 100_000, 0.05)}


def rows(S, L, het, seed):
    g = np.random.default_rng(seed)
    d = (g.random((S, L), dtype=np.float32) < het).astype(np.int8)
    d.flat[g.integers(0, d.size, size=int(0.01 * d.size))] = -1
    d[:, 0] = 1
    return d


def timed(fns, reps):
    """medians (ms) of ``reps`` alternating calls of every function after one warm-up call of each"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bckd")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from phlash_amd import _lib
    from phlash_amd.engine import HipEngine
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population
    import pair_count_bars as bars
    import pair_count_oracle as pco
    from oracle import psmc_numpy as pn

    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    for key in args.shapes:
        K, dbl, B, S, L, het = SHAPES[key]
        data = rows(S, L, het, seed=7)
        tmpl, x = particle_population(K, B, seed=1, sigma=0.25)
        pp = PSMCParams.from_dm(tmpl.from_flat(x).to_dm())
        P = pp.stack()[:, None].cuda()  # [B, 1, 7, K] float64
        eng = HipEngine(K, data, double_precision=dbl)
        inds = torch.arange(S, device="cuda")
        ll, c = eng.pair_counts(P, inds, 0)
        assert not eng.underflow_risk()
        assert torch.isfinite(c).all()
        ll0, _, _ = eng.posterior(P, inds, 0, bin=100, marginals=True)
        assert torch.equal(ll, ll0)
        worst = 0.0
        for b, s in ((0, 0), (B - 1, S - 1)):
            q = pn.PP(*(getattr(pp, name)[b].numpy() for name in pn.PP._fields))
            ref, llr = pco.pair_counts(q, data[s], 0)
            worst = max(worst, pco.error(c[b, s].cpu().numpy(), ref))
            assert abs(float(ll[b, s]) / llr - 1) < (1e-12 if dbl else 1e-5)
        assert worst < (bars.F64_COUNTS_BAR if dbl else max(bars.F32_COUNTS_BAR, bars.F32_LONG_ROW_BAR)), worst
        check = f"counts vs float64 oracle on 2 sequences: max |C - oracle| / max(1, oracle) {worst:.1e}; ll bitwise phk_posterior's"
        del c
        t_pc, t_tr, t_dec = timed([lambda: eng.pair_counts(P, inds, 0),
                                   lambda: eng.transitions(P, inds, 0, bin=100, arrivals=True, changes=True),
                                   lambda: eng.posterior(P, inds, 0, bin=100, marginals=True)], args.reps)
        print(json.dumps({"shape": key, "K": K, "float64": dbl, "B": B, "S": S, "L": L, "het": het, "pair_counts_ms": round(t_pc, 3),
                          "transitions_ms": round(t_tr, 3), "posterior_ms": round(t_dec, 3), "vs_transitions": round(t_pc / t_tr, 3),
                          "vs_posterior": round(t_pc / t_dec, 3), "check": check, "lib_sha256": sha}), flush=True)
        del eng, ll
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
