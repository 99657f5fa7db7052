"""HIP-event time of a bin-moment call (bin = 1 and bin = 100) against a tract-posterior call and a posterior-decoding call (mean
track) at the same bin on the same inputs, K = 16, float32 kernels (not run by bench.py).

Shapes: (b) 100 models x 20 rows x 100,000 windows; (c) the reference's production shape, 500 x 5 x 100,000; both at 5 % hets.
Before it reports a shape the script checks the two moments against the float64 dense oracle of tests/moment_oracle.py on two
(model, row) pairs, and prints one JSON line per shape and bin with the library's sha256.

    python scripts/moments_timing.py [--shapes bc] [--bins 1,100] [--reps 5]
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

SHAPES = {"b": (100, 20, 100_000, 0.05), "c": (500, 5, 100_000, 0.05)}


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
    ap.add_argument("--bins", default="1,100")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from phlash_amd import _lib
    from phlash_amd.engine import HipEngine
    from phlash_amd.params import PSMCParams
    from phlash_amd.synth import particle_population
    import moment_bars as bars
    import moment_oracle as mo
    from oracle import psmc_numpy as pn

    sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    m = (np.arange(16) < 11).astype(np.float64)  # the tract call's weights: the eleven youngest states
    for key in args.shapes:
        B, S, L, het = SHAPES[key]
        data = rows(S, L, het, seed=7)
        tmpl, x = particle_population(16, B, seed=1, sigma=0.25)
        dm = tmpl.from_flat(x).to_dm()
        pp = PSMCParams.from_dm(dm)
        P = pp.stack()[:, None].cuda()  # [B, 1, 7, K] float64
        ect = torch.as_tensor(dm.eta.ect(), dtype=torch.float64).reshape(-1, 16).expand(B, 16).contiguous()
        # the moment call's values: every model's expected coalescence times, centred by its prior mean and scaled into [-1, 1]
        pi = torch.as_tensor(pp.pi, dtype=torch.float64).reshape(B, 16)
        c = (ect * pi).sum(-1, keepdim=True) / pi.sum(-1, keepdim=True)
        v = ((ect - c) / (ect - c).abs().max(-1, keepdim=True).values).contiguous()
        f, w, vd = ect.cuda(), torch.as_tensor(m).cuda(), v.cuda()
        eng = HipEngine(16, data, double_precision=False)
        inds = torch.arange(S, device="cuda")
        for bin in (int(b) for b in args.bins.split(",")):
            ll, m1, m2 = eng.bin_moments(P, inds, vd, 0, bin=bin)
            assert not eng.underflow_risk()
            assert torch.isfinite(m1).all() and torch.isfinite(m2).all()
            ll0, _, _ = eng.posterior(P, inds, 0, values=f, bin=bin, marginals=False, mean=True)
            assert torch.equal(ll, ll0)
            w1 = w2 = 0.0
            for b, s in ((0, 0), (B - 1, S - 1)):
                q = pn.PP(*(getattr(pp, name)[b].numpy() for name in pn.PP._fields))
                r1, r2, llr = mo.dense(q, data[s], v[b].numpy(), 0, bin)
                w1 = max(w1, float((np.abs(m1[b, s].cpu().numpy() - r1) / np.maximum(1.0, np.abs(r1))).max()))
                w2 = max(w2, float((np.abs(m2[b, s].cpu().numpy() - r2) / np.maximum(1.0, r2)).max()))
                assert abs(float(ll[b, s]) / llr - 1) < 1e-5
            print(f"# shape {key} bin {bin}: m1 {w1:.3e} m2 {w2:.3e} against the oracle", file=sys.stderr, flush=True)
            assert max(w1, w2) < bars.F32_MOMENT_BAR[16], (w1, w2)
            sd = torch.sqrt((m2 - m1 * m1).clamp(min=0))
            check = (f"moments vs float64 oracle on 2 sequences: m1 {w1:.1e}, m2 {w2:.1e} in units of max(1, |.|) "
                     f"(mean sd of the bin sum {float(sd.mean()):.3f}); ll bitwise phk_posterior's")
            t_mo, t_tr, t_dec = timed([lambda: eng.bin_moments(P, inds, vd, 0, bin=bin), lambda: eng.tracts(P, inds, w, 0, bin=bin),
                                       lambda: eng.posterior(P, inds, 0, values=f, bin=bin, marginals=False, mean=True)], args.reps)
            print(json.dumps({"shape": key, "B": B, "S": S, "L": L, "het": het, "bin": bin, "moments_ms": round(t_mo, 3),
                              "tracts_ms": round(t_tr, 3), "posterior_ms": round(t_dec, 3), "ratio_to_tracts": round(t_mo / t_tr, 3),
                              "ratio_to_posterior": round(t_mo / t_dec, 3), "plan": eng.get_plan(), "check": check, "lib_sha256": sha}), flush=True)
            del m1, m2, ll
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
