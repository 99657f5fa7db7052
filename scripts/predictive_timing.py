"""HIP-event time of a leave-one-out predictive call (bin = 1) against a posterior-decoding call (mean track, bin = 1) on the
same inputs, K = 16, float32 kernels (not run by bench.py).

Shapes: (b) 100 models x 20 rows x 100,000 windows; (c) the reference's production shape, 500 x 5 x 100,000 at 5 % hets.
Before it reports a shape the script checks the track against the float64 dense oracle of tests/predictive_oracle.py on
two (model, row) pairs, and prints one JSON line per shape with the library's sha256.

    python scripts/predictive_timing.py [--shapes bc] [--reps 5]
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
    import predictive_bars as bars
    import predictive_oracle as lo
    from oracle import psmc_numpy as pn

    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    for key in args.shapes:
        B, S, L, het = SHAPES[key]
        data = rows(S, L, het, seed=7)
        tmpl, x = particle_population(16, B, seed=1, sigma=0.25)
        dm = tmpl.from_flat(x).to_dm()
        pp = PSMCParams.from_dm(dm)
        P = pp.stack()[:, None].cuda()  # [B, 1, 7, K] float64
        f = torch.as_tensor(dm.eta.ect(), dtype=torch.float64).reshape(-1, 16).expand(B, 16).contiguous().cuda()
        eng = HipEngine(16, data, double_precision=False)
        inds = torch.arange(S, device="cuda")
        ll, trk = eng.predictive(P, inds, 0, bin=1)
        assert not eng.underflow_risk()
        assert torch.isfinite(trk).all()
        ll0, _, _ = eng.posterior(P, inds, 0, values=f, bin=1, marginals=False, mean=True)
        assert torch.equal(ll, ll0)
        worst_h = worst_s = 0.0
        for b, s in ((0, 0), (B - 1, S - 1)):
            q = pn.PP(*(getattr(pp, name)[b].numpy() for name in pn.PP._fields))
            ph, sc, llr = lo.loo(q, data[s], 0)
            ref = lo.reduce_bins(ph, sc, data[s], 0, 1)  # [L, 3]
            got = trk[b, s].double().cpu().numpy()
            worst_h = max(worst_h, float(np.abs(got[:, :2] - ref[:, :2]).max()))
            worst_s = max(worst_s, float((np.abs(got[:, 2] - ref[:, 2]) / np.maximum(1.0, np.abs(ref[:, 2]))).max()))
            assert abs(float(ll[b, s]) / llr - 1) < 1e-5
        assert worst_h < bars.F32_HET_BAR and worst_s < bars.F32_SCORE_BAR, (worst_h, worst_s)
        check = f"track vs float64 oracle on 2 sequences: het max abs {worst_h:.1e}, score rel {worst_s:.1e}; ll bitwise phk_posterior's"
        t_lo, t_dec = timed_pair(lambda: eng.predictive(P, inds, 0, bin=1),
                                 lambda: eng.posterior(P, inds, 0, values=f, bin=1, marginals=False, mean=True), args.reps)
        print(json.dumps({"shape": key, "B": B, "S": S, "L": L, "het": het, "predictive_ms": round(t_lo, 3), "posterior_ms": round(t_dec, 3),
                          "ratio": round(t_lo / t_dec, 3), "plan": eng.get_plan(), "check": check, "lib_sha256": sha}), flush=True)
        del eng, trk, ll
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
